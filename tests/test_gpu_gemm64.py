"""Every GEMM tile and epilogue against float64, element by element (tests/_gemm64.py: the reference and its per-element bound).

The cases are the engines' production shapes -- SD1.5 / SDXL convs and linears, DiT-XL/2's projections, the VAE's convs and
attention products -- plus the few shapes that reach an instantiation no production shape does.  Each runs through
engine.op_gemm (dsim_op_gemm: the whole GemmArgs surface) in all three dtypes and checks
  * the bound on every element (or on tests/_gemm64.row_subset's rows: every M tile's first and last row, both sides of every image
    and rows_per_batch boundary, a random sample);
  * that every element is finite, and that nothing is written outside the output: guard rows past M, columns N..ldo, the gaps
    between out_split tensors;
  * gn_part: the partial sums against float64 sums of the STORED output, op_groupnorm_pre against float64 GroupNorm + SiLU of
    the stored output and against op_groupnorm on the same input;
  * the small-batch kernel: bit for bit the rows of a large-M launch of the same problem on the regular tiles.
test_launch_coverage then holds the launch records of the whole case list to the table of every instantiation gemm_plan can
name on MI355X (256 CUs), and gemm_family's names to the records."""
import math
import time

import pytest
import torch
import torch.nn.functional as F

from tests import _gemm64 as G

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
SENT = -12345.0              # fill of the output buffer: what the kernel must leave alone


def _lin(M, C0, N, **kw):
    return dict(M=M, C0=C0, N=N, **kw)


def _conv(B, H, W, C0, N, **kw):
    return dict(conv=dict(stride=kw.pop("stride", 1), ups=kw.pop("ups", 0), pad=kw.pop("pad", 1)), B=B, H=H, W=W, C0=C0, N=N, **kw)


# name -> problem.  Keys: linear M / C0 (/ C1: the A1 concatenation) or conv B, H, W, C0 (+ stride / ups / pad); N weight rows;
# res, bias2 (rows_per_batch), act, gate (+ gate2, rows_per_batch; with res), geglu, ldo_pad, split (out_split), big (force_big),
# wb (wb_rows), gn (gn_part, 16-bit only), sub (reference a row subset).
CASES = {
    # ---- SD1.5 / SDXL 3x3 convs: the 64 / 32 / 16 / 8 levels, odd sides 28 / 14 / 7, stride 2, upsample, per-half bias
    "sd_conv320_64": _conv(4, 64, 64, 320, 320, sub=1),                       # 128 x 80 (16-bit)
    "sd_conv320_64_res": _conv(4, 64, 64, 320, 320, res=1, sub=1),
    "sd_conv320_64_b8": _conv(8, 64, 64, 320, 320, sub=1),                    # 128 x 160
    "sd_conv320_64_b8_res": _conv(8, 64, 64, 320, 320, res=1, sub=1),
    "sd_conv640_32_big": _conv(4, 32, 32, 640, 640, big=1),                   # 256 x 320 conv3p
    "sd_conv640_32_big_res": _conv(4, 32, 32, 640, 640, big=1, res=1),
    "sd_conv1280_16": _conv(4, 16, 16, 1280, 1280),                           # small-batch 64 x 80
    "sd_conv1280_16_res": _conv(4, 16, 16, 1280, 1280, res=1),
    "sd_conv1280_8": _conv(4, 8, 8, 1280, 1280),                              # small-batch 64 x 64
    "sd_conv1280_8_res": _conv(4, 8, 8, 1280, 1280, res=1),
    "sd_conv1280_16_b5_res": _conv(5, 16, 16, 1280, 1280, res=1),            # small-batch 64 x 128
    "sd_conv1280_16_b8": _conv(8, 16, 16, 1280, 1280),                        # small-batch 128 x 80
    "sd_conv1280_16_b8_res": _conv(8, 16, 16, 1280, 1280, res=1),
    "sd_conv1280_16_b10_res": _conv(10, 16, 16, 1280, 1280, res=1),          # small-batch 128 x 128
    "sd_conv320_64_s2": _conv(4, 64, 64, 320, 320, stride=2),
    "sd_conv640_28_s2": _conv(4, 28, 28, 640, 640, stride=2),                 # 28 -> 14
    "sd_conv640_28_s2_big": _conv(4, 28, 28, 640, 640, stride=2, big=1),      # 256 x 320 conv3 (14 x 14)
    "sd_conv1280_14_s2": _conv(4, 14, 14, 1280, 1280, stride=2),              # 14 -> 7
    "sd_conv1280_up8": _conv(4, 8, 8, 1280, 1280, ups=1),
    "sd_conv640_up16_big": _conv(4, 16, 16, 640, 640, ups=1, big=1),
    "sd_conv640_28_big_res": _conv(4, 28, 28, 640, 640, big=1, res=1),       # 256 x 320 conv3, residual
    "xl_conv1280_14_bias2": _conv(4, 14, 14, 1280, 1280, bias2=196),        # small-batch, tiles straddle the 196-row elements
    "xl_conv1280_7_bias2": _conv(8, 7, 7, 1280, 1280, bias2=49),
    "xl_conv640_14_bias2_big": _conv(8, 14, 14, 640, 640, bias2=196, big=1),  # 256 x 320 conv3 straddling elements
    "xl_conv640_7_bias2_ldo": _conv(4, 7, 7, 640, 640, bias2=49, ldo_pad=8),
    # ---- U-Net linears: the concatenated A1 shortcut, tapped q | k | v, GEGLU with both block sizes, widths 320 .. 1280
    "unet_shortcut_concat": _lin(4096, 1280, 640, C1=640),                  # small-batch 128 x 80
    "unet_shortcut_concat_res": _lin(4096, 1280, 640, C1=640, res=1),
    "unet_linear320_80": _lin(16384, 320, 320, ldo_pad=8),                    # 128 x 80 (K < 512: no small-batch kernel)
    "unet_linear320_80_res": _lin(16384, 320, 320, res=1),
    "unet_linear320_160": _lin(32768, 320, 320, sub=1),                       # 128 x 160
    "unet_linear320_160_res": _lin(32768, 320, 320, res=1, sub=1),
    "unet_linear640_big": _lin(4096, 640, 640, big=1),                        # 256 x 320
    "unet_linear640_big_res": _lin(4096, 640, 640, big=1, res=1, ldo_pad=8),
    "unet_linear1280_8": _lin(256, 1280, 1280),                               # small-batch 64 x 64
    "unet_linear1280_8_res": _lin(256, 1280, 1280, res=1),
    "unet_linear1280_16": _lin(1024, 1280, 1280),                             # small-batch 64 x 80
    "unet_linear1280_16_res": _lin(1024, 1280, 1280, res=1),
    "unet_linear1280_b5": _lin(1280, 1280, 1280),                             # small-batch 64 x 128
    "unet_linear1280_b5_res": _lin(1280, 1280, 1280, res=1),
    "unet_linear1280_b10": _lin(2560, 1280, 1280),                            # small-batch 128 x 128
    "unet_linear1280_b10_res": _lin(2560, 1280, 1280, res=1),
    "unet_qkv320": _lin(16384, 320, 960, split=320, ldo_pad=8),              # tapped q | k | v, gaps between the three
    "unet_qkv640": _lin(4096, 640, 1920, split=640),
    "unet_qkv1280": _lin(1024, 1280, 3840, split=1280, ldo_pad=8),
    "unet_geglu320": _lin(16384, 320, 2560, geglu=1),                         # 32-row blocks, 256 x 256
    "unet_geglu320_small": _lin(1024, 320, 2560, geglu=1),                    # 32-row blocks, 128 x 128
    "unet_geglu640": _lin(4096, 640, 5120, geglu=1),                          # 16-row blocks, 256 x 320
    "unet_geglu1280": _lin(1024, 1280, 10240, geglu=1, ldo_pad=8),            # 16-row blocks, 128 x 160
    # ---- DiT-XL/2 (hidden 1152): fc1 tanh-GELU, gated residual proj / fc2 at T = 256 and 196, qkv 3456
    "dit_fc1_t256": _lin(8192, 1152, 4608, act=1, sub=1),                     # 256 x 320 tanh-GELU (ragged last column tile)
    "dit_fc1_small": _lin(512, 1152, 4608, act=1),                            # 128 x 128
    "dit_proj_t256_gate": _lin(11264, 1152, 1152, gate=256, res=1, sub=1),    # 256 x 192
    "dit_fc2_t196_gate": _lin(10976, 4608, 1152, gate=196, res=1, sub=1),     # 256 x 192, per-row CFG parity (196 % 16 != 0)
    "dit_proj_t196_gate_small": _lin(784, 1152, 1152, gate=196, res=1),       # 128 x 128
    "dit_fc2_t256_gate_small": _lin(512, 4608, 1152, gate=256, res=1),
    "dit_qkv_t256_big": _lin(16384, 1152, 3456, sub=1),                       # ragged 256 x 320
    "dit_qkv_t256": _lin(8192, 1152, 3456, sub=1),                            # ragged 256 x 256
    "dit_qkv_small": _lin(2048, 1152, 3456),                                  # 128 x 128
    "dit_qkv_one_image": _lin(512, 1152, 3456),                               # small-batch 64 x 128
    "dit_proj_nogate": _lin(12288, 1152, 1152, sub=1),                        # 256 x 192 plain
    "dit_proj_nogate_res": _lin(12288, 1152, 1152, res=1, sub=1),
    "dit_proj_small": _lin(2048, 1152, 1152),                                 # 128 x 128
    "dit_proj_small_res": _lin(2048, 1152, 1152, res=1),
    # (reachable, not production: tanh-GELU on 256 x 192 / 256 x 256, the gate on 256 x 256)
    "act_n1152_big": _lin(2048, 1152, 1152, act=1, big=1),
    "act_n3456": _lin(6144, 1152, 3456, act=1, sub=1),
    "gate_n3456": _lin(4864, 1152, 3456, gate=256, res=1, sub=1),
    # ---- VAE: pad 0 stride-2 downsamples, the per-image attention products, force_big, GroupNorm statistics epilogues
    "vae_down_512": _conv(1, 512, 512, 128, 128, stride=2, pad=0, sub=1),   # 256 x 128 conv3p
    "vae_down_256": _conv(1, 256, 256, 256, 256, stride=2, pad=0),           # small-batch 128 x 128
    "vae_down_128": _conv(1, 128, 128, 512, 512, stride=2, pad=0),           # small-batch 64 x 128
    "vae_qkT_512": _lin(8192, 512, 4096, wb=4096, sub=1),                     # 256 x 256, per-image weights
    "vae_proj_out_big_res": _lin(4096, 512, 512, res=1, big=1),             # 256 x 256 residual
    "vae_qkT_256": _lin(2048, 512, 1024, wb=1024),                            # 128 x 128
    "vae_pv_256": _lin(2048, 1024, 512, wb=1024),
    "vae_conv512_128_big": _conv(1, 128, 128, 512, 512, big=1, sub=1),       # 256 x 256 conv3p
    "vae_conv512_128_big_res": _conv(1, 128, 128, 512, 512, big=1, res=1, sub=1),
    "vae_conv256_96_big": _conv(1, 96, 96, 256, 256, big=1),                  # 256 x 256 conv3 (not a power of two)
    "vae_conv256_96_big_res": _conv(1, 96, 96, 256, 256, big=1, res=1),
    "vae_conv128_150": _conv(3, 150, 150, 128, 128, sub=1),                  # 256 x 128 conv3
    "vae_conv128_150_res": _conv(3, 150, 150, 128, 128, res=1, sub=1),
    "vae_conv128_128_b3": _conv(3, 128, 128, 128, 128, sub=1),               # 128 x 128 conv3
    "vae_conv128_128_b3_res": _conv(3, 128, 128, 128, 128, res=1, sub=1),
}
for _side, _c in ((512, 128), (256, 128), (256, 256)):                     # 512 x 128, 256 x 128, 256 x 256: plain, residual, +gn_part
    for _res in (0, 1):
        for _gn in (0, 1):
            CASES[f"vae_conv{_c}_{_side}{'_res' if _res else ''}{'_gn' if _gn else ''}"] = _conv(1, _side, _side, _c, _c, res=_res, gn=_gn,
                                                                                              sub=1)

# (dtype, small, bm, bn, kind, geglu, ek) of every instantiation gemm_plan can name on a 256-CU MI355X
_H16 = ([(0, 512, 128, "conv3p", 0, ek) for ek in ("plain", "residual", "plain_gn", "residual_gn")]
        + [(0, 256, bn, "conv3p", 0, ek) for bn in (128, 256) for ek in ("plain", "residual", "plain_gn", "residual_gn")]
        + [(0, 256, bn, kind, 0, ek) for bn, kind in ((320, "conv3p"), (320, "conv3"), (256, "conv3"), (128, "conv3"))
           for ek in ("plain", "residual")]
        + [(0, 256, 320, "linear", 1, "plain"), (0, 256, 256, "linear", 1, "plain")]
        + [(0, 256, bn, "linear", 0, ek) for bn in (320, 256, 192) for ek in ("plain", "residual")]
        + [(0, 256, 320, "linear", 0, "act")]
        + [(0, 256, bn, "linear", 0, ek) for bn in (256, 192) for ek in ("act", "dit")]
        + [(0, 128, 128, "linear", 0, ek) for ek in ("act", "dit")]
        + [(0, 128, bn, "linear", 1, "plain") for bn in (160, 128)]
        + [(0, 128, bn, kind, 0, ek) for bn in (160, 128, 80) for kind in ("linear", "conv3") for ek in ("plain", "residual")]
        + [(1, bm, bn, kind, 0, ek) for bm, bn in ((64, 64), (64, 80), (64, 128), (128, 80), (128, 128))
           for kind in ("linear", "conv3") for ek in ("plain", "residual")])
_F32 = ([(0, 128, 128, "linear", 0, ek) for ek in ("act", "dit")]
        + [(0, 128, bn, "linear", 1, "plain") for bn in (160, 128)]
        + [(0, 128, bn, kind, 0, ek) for bn in (160, 128) for kind in ("linear", "conv3") for ek in ("plain", "residual")])
REACHABLE = {"bf16": set(_H16), "f16": set(_H16), "f32": set(_F32)}
# Instantiations the product library compiles that no arguments reach: none.  gemm.hip's gemm_compiled() and common.h's kSkinnyTiles
# state the compiled set, gemm_plan() plans inside it, and the one tile no plan of the product names (the small-batch 128 x 64) is
# compiled, like 128 x 160, in -DDSIM_DEVTOOLS builds only, where g_skinny_tile selects it.  tests/test_gemm64_host.py holds
# REACHABLE | UNREACHABLE to the kernel symbols of the built library, so a new instantiation cannot go unlisted.
_UNREACHED_H16 = []
UNREACHABLE = {"bf16": set(_UNREACHED_H16), "f16": set(_UNREACHED_H16), "f32": set()}

RECORDS = {}                 # (case, dtype) -> launch record


def _gen(shape, g, scale=1.0):
    return torch.randn(*shape, generator=g, device="cuda") * scale


def _problem(name, dt):
    """inputs of case `name` in dtype dt (seeded), and the op_gemm keyword arguments"""
    c = CASES[name]
    dtype = DT[dt]
    g = torch.Generator(device="cuda").manual_seed(sum(map(ord, name)))
    N, C0, C1 = c["N"], c["C0"], c.get("C1", 0)
    if "conv" in c:
        a0 = _gen((c["B"], c["H"], c["W"], C0), g).to(dtype)
        Ho, Wo = G.conv_out_hw(c["H"], c["W"], **c["conv"])
        M, K = c["B"] * Ho * Wo, 9 * C0
        w = _gen((N, C0, 3, 3), g, 1 / math.sqrt(K))
        a1 = None
    else:
        M, K = c["M"], C0 + C1
        a0 = _gen((M, C0), g).to(dtype)
        a1 = _gen((M, C1), g).to(dtype) if C1 else None
        w = _gen(((M // c["wb"]) if c.get("wb") else 1, N, K), g, 1 / math.sqrt(K))
        w = w if c.get("wb") else w[0]
    geglu = c.get("geglu", 0)
    ncol = N // 2 if geglu else N
    split = c.get("split", 0)
    ldo = (split or ncol) + c.get("ldo_pad", 0)
    kw = dict(a1=a1, conv=c.get("conv"), bias=_gen((N,), g, 0.5), epi="geglu" if geglu else ("residual" if c.get("res") else "none"),
              ldo=ldo, force_big=c.get("big", 0))
    if c.get("bias2"):
        kw.update(bias2=_gen((N,), g, 0.5), rows_per_batch=c["bias2"])
    if c.get("act"):
        kw["act"] = 1
    if c.get("gate"):
        kw.update(gate=_gen((ncol,), g), gate2=_gen((ncol,), g), rows_per_batch=c["gate"])
    if c.get("res"):
        kw["residual"] = _gen((M, ldo), g).to(dtype)
    if c.get("wb"):
        kw.update(wb_rows=c["wb"], wb_stride=N * K * dtype.itemsize + 256)
    if split:
        kw.update(out_split=split, out_split_stride=(M * ldo + 512) * dtype.itemsize)
    if c.get("gn"):
        hw = Ho * Wo
        kw.update(gn_part=torch.full((c["B"], hw // 64, N // 4, 2), float("nan"), device="cuda"), gn_hw=hw)
    return dict(a0=a0, w=w, M=M, K=K, N=N, ncol=ncol, ldo=ldo, split=split, dtype=dtype, kw=kw)


def _outbuf(p):
    """the output buffer: M rows of ldo (per out_split tensor, 512-element gaps between them) plus 4 guard rows, all SENT"""
    nout = p["N"] // p["split"] if p["split"] else 1
    per = p["M"] * p["ldo"] + (512 if p["split"] else 0)
    return torch.full((nout * per + 4 * p["ldo"],), SENT, dtype=p["dtype"], device="cuda"), nout, per


def _launch(name, dt):
    p = _problem(name, dt)
    out, nout, per = _outbuf(p)
    rec = _eng().op_gemm(p["a0"], p["w"], out, **p["kw"])
    torch.cuda.synchronize()
    RECORDS[(name, dt)] = rec
    return p, out, nout, per, rec


def _eng():
    from diffsim_amd import engine
    return engine


def _outputs(p, out, nout, per):
    """[M][ncol] as the model sees it (the out_split tensors side by side), and the guard check"""
    M, ldo = p["M"], p["ldo"]
    sent = torch.tensor(SENT, dtype=p["dtype"])
    cols = p["split"] or p["ncol"]
    parts = []
    for j in range(nout):
        blk = out[j * per: j * per + M * ldo].view(M, ldo)
        parts.append(blk[:, :cols])
        assert (blk[:, cols:].cpu() == sent).all(), f"written in columns {cols}..{ldo}"
        assert (out[j * per + M * ldo: (j + 1) * per].cpu() == sent).all(), "written between out_split tensors"
    assert (out[nout * per:].cpu() == sent).all(), "written past row M"
    return torch.cat(parts, 1)


def _reference(name, p, rec, rows=None):
    c, kw = CASES[name], p["kw"]
    if rows is None and c.get("sub"):
        bnd = []
        if kw.get("rows_per_batch"):
            bnd += list(range(kw["rows_per_batch"], p["M"], kw["rows_per_batch"]))
        if "conv" in c:
            bnd += list(range(p["M"] // c["B"], p["M"], p["M"] // c["B"]))
        if c.get("wb"):
            bnd += list(range(c["wb"], p["M"], c["wb"]))
        rows = G.row_subset(p["M"], rec["bm"], bnd, n_random=256)
    return G.Gemm64(p["a0"], p["w"], p["dtype"], a1=kw.get("a1"), conv=kw.get("conv"), bias=kw.get("bias"), bias2=kw.get("bias2"),
                    rows_per_batch=kw.get("rows_per_batch", 0), act=kw.get("act", 0), gate=kw.get("gate"), gate2=kw.get("gate2"),
                    epi=kw["epi"], residual=kw.get("residual"), wb_rows=kw.get("wb_rows", 0), rows=rows)


WORST = {}                   # (case, dtype) -> largest err / bound (printed by test_launch_coverage)


def _check_gn(name, p, got, kw):
    c = CASES[name]
    B, hw, N = c["B"], kw["gn_hw"], p["N"]
    part = kw["gn_part"]
    assert torch.isfinite(part).all(), "gn_part slots left unwritten"
    x = got.double().view(B, hw // 64, 64, N // 4, 4)
    s1, s2 = x.sum((2, 4)), (x * x).sum((2, 4))
    a1, a2 = x.abs().sum((2, 4)), (x * x).sum((2, 4))
    # f32 sums of 256 terms: worst case 256 u32 sum|x|
    assert ((part[..., 0].double() - s1).abs() <= 256 * G.U32 * a1 + 1e-30).all(), "gn_part sums"
    assert ((part[..., 1].double() - s2).abs() <= 256 * G.U32 * a2 + 1e-30).all(), "gn_part sums of squares"
    gen = torch.Generator(device="cuda").manual_seed(7)
    gamma, beta = 1 + 0.1 * _gen((N,), gen), 0.1 * _gen((N,), gen)
    xin = got.view(B, hw, N)
    pre = _eng().op_groupnorm_pre(xin, gamma, beta, 32, 1e-6, True, part, hw // 64)
    ref = F.silu(F.group_norm(xin.double().permute(0, 2, 1), 32, gamma.double(), beta.double(), 1e-6)).permute(0, 2, 1)
    u = G.U[p["dtype"]]
    # one rounding to the output, plus the f32 statistics (64-row partials folded in f64) and the f32 affine: 1e-5 of the
    # normalised magnitude
    bound = u * ref.abs() + 1e-5 * (ref.abs() + 1.0)
    assert ((pre.double() - ref).abs() <= bound).all(), "op_groupnorm_pre against float64 GroupNorm + SiLU"
    # and tests/_norm64.py's bound for the statistics-epilogue form.  Both asserts stay: the derived bound is not everywhere the
    # smaller of the two (tests/test_norm64_host.py test_derived_bound_against_the_hand_set_one compares them)
    from tests import _norm64 as N64
    plan = _eng().groupnorm_plan(N, 0, B, hw, 32, p["dtype"], pre=True)
    r64, b64 = N64.gn_ref_and_bound(xin, None, gamma, beta, 32, 1e-6, True, p["dtype"], N64.gn_n_p(plan, hw))
    N64.check(pre, r64, b64, f"op_groupnorm_pre within tests/_norm64.py's bound {plan}")
    plain = _eng().op_groupnorm(xin, None, gamma, beta, 32, 1e-6, True)
    assert ((pre.double() - plain.double()).abs() <= 2 * u * plain.double().abs() + 2e-5).all(), "op_groupnorm_pre against op_groupnorm"


def _bigger(name, p, rep):
    """the same problem with its rows repeated `rep` times (images for a conv): the regular tiles' launch of the same rows"""
    kw = dict(p["kw"])
    if kw.get("a1") is not None:
        kw["a1"] = kw["a1"].repeat(rep, 1)
    if kw.get("residual") is not None:
        kw["residual"] = kw["residual"].repeat(rep, 1)
    q = dict(p, M=p["M"] * rep, kw=kw)
    out, nout, per = _outbuf(q)
    rec = _eng().op_gemm(p["a0"].repeat(rep, *([1] * (p["a0"].ndim - 1))), p["w"], out, **kw)
    return rec, _outputs(q, out, nout, per)[: p["M"]]


def _runs():
    """(case, dtype) pairs: every case in every dtype, but the statistics epilogue in the 16-bit ones only"""
    return [(name, dt) for name, c in CASES.items() for dt in DT if not (c.get("gn") and dt == "f32")]


@pytest.mark.parametrize("name,dt", _runs())
def test_gemm_against_float64(name, dt):
    c = CASES[name]
    p, out, nout, per, rec = _launch(name, dt)
    got = _outputs(p, out, nout, per)
    assert torch.isfinite(got.float()).all(), "non-finite output"
    ref = _reference(name, p, rec)
    WORST[(name, dt)] = ref.check(got[ref.rows.cuda()], f"{name} {dt} {rec['family']}")
    if c.get("gn"):
        _check_gn(name, p, got, p["kw"])
    if rec["small"]:
        rep = max(2, -(-16384 // p["M"]))
        brec, big = _bigger(name, p, rep)
        assert not brec["small"], brec
        assert torch.equal(big.view(torch.int16 if p["dtype"] != torch.float32 else torch.int32),
                           got.view(torch.int16 if p["dtype"] != torch.float32 else torch.int32)), \
            f"small-batch kernel differs from the regular tiles ({brec['family']})"


def _family_fields(fam):
    """(small, bm, bn, kind, geglu, residual, gn, act, dit) from a gemm_family() name"""
    head = fam.split("|")[0].split("_")
    small = head[1] == "small"
    f = head[2:] if small else head[1:]
    bm, bn = (int(v) for v in f[1].split("x"))
    return small, bm, bn, f[2], "geglu" in f[3:], "res" in f[3:], "gn" in f[3:], "act" in f[3:], "dit" in f[3:]


def test_launch_coverage():
    """The launch records of the case list equal the table of reachable instantiations, per dtype; gemm_family names the kernel
    and tile that ran for every case.  (Cases not run in this session are launched here, without the reference.)"""
    t0 = time.time()
    for name, dt in _runs():
        if (name, dt) not in RECORDS:
            _launch(name, dt)
    seen = {dt: set() for dt in DT}
    for (name, dt), r in RECORDS.items():
        key = (int(r["small"]), r["bm"], r["bn"], r["kind"], int(r["geglu"]), r["ek"])
        seen[dt].add(key)
        small, bm, bn, kind, geglu, res, gn, act, dit = _family_fields(r["family"])
        assert (small, bm, bn, kind, geglu) == (r["small"], r["bm"], r["bn"], r["kind"], r["geglu"]), (name, dt, r)
        assert (act, dit) == (r["ek"] == "act", r["ek"] == "dit"), (name, dt, r)
        if r["ek"] in ("plain", "residual", "plain_gn", "residual_gn"):
            assert (res, gn) == (r["ek"].startswith("residual"), r["ek"].endswith("_gn")), (name, dt, r)
    for dt in DT:
        assert seen[dt] == REACHABLE[dt], (dt, "missing", sorted(REACHABLE[dt] - seen[dt]), "unexpected", sorted(seen[dt] - REACHABLE[dt]))
    fams = {}
    for (name, dt), w in WORST.items():
        fam = RECORDS[(name, dt)]["family"].split("|")[0].replace(f"_{dt}_", "_")
        fams[(fam, dt)] = max(fams.get((fam, dt), 0.0), w)
    for k in sorted(fams):
        print(f"worst err/bound {k[1]:4s} {k[0]:28s} {fams[k]:.3f}")
    print(f"coverage pass {time.time() - t0:.1f} s")


def test_op_gemm_refuses_inconsistent_arguments():
    """dsim_op_gemm's own checks (a C caller gets no engine.op_gemm in front): bias2 / gate2 without bias / gate, ldo below the
    output width; dsim_op_groupnorm_pre: chunks other than HW / 64"""
    from diffsim_amd import _lib
    eng = _eng()
    M, K, N = 256, 128, 128
    x = torch.randn(M, K, device="cuda").to(torch.bfloat16)
    w = torch.randn(N, K, device="cuda")
    v = torch.randn(N, device="cuda")
    out = torch.zeros(M * N, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(_lib.DsimError):
        eng.op_gemm(x, w, out, bias2=v, rows_per_batch=64)
    with pytest.raises(_lib.DsimError):
        eng.op_gemm(x, w, out, bias=v, gate2=v, rows_per_batch=64)
    op = _lib.GemmOpC()
    op.A0, op.C0, op.M, op.N, op.K, op.w, op.out, op.ldo, op.dtype = x.data_ptr(), K, M, N, K, w.data_ptr(), out.data_ptr(), N - 8, 1
    rec = _lib.GemmLaunchC()
    import ctypes
    assert _lib.lib().dsim_op_gemm(ctypes.byref(op), ctypes.byref(rec), None) == -1
    assert (out == 0).all()
    xg = torch.randn(1, 128, 64, device="cuda").to(torch.bfloat16)
    g, b = torch.ones(64, device="cuda"), torch.zeros(64, device="cuda")
    with pytest.raises(_lib.DsimError):
        eng.op_groupnorm_pre(xg, g, b, 16, 1e-6, True, torch.zeros(1, 1, 16, 2, device="cuda"), 1)
