"""Every normalization kernel against float64, element by element (tests/_norm64.py: the reference and its per-element bound).

The cases are every distinct GroupNorm (HW, C0, C1, groups, silu, eps) the SD1.5 / SDXL executors (csrc/unet.hip resnet() /
transformer(): norm_eps = 1e-5 with SiLU, 1e-6 without) and the VAE encoder (csrc/vae.hip: eps 1e-6) issue at 512 px and at 224 px,
every LayerNorm (M, C) of the U-Nets, DiT's modulated LayerNorm (csrc/dit.hip lnmod: eps 1e-6, rows_per_batch = T), the shapes that
reach a dispatch arm no production shape does, and input families beyond randn (FAMILIES).  Each runs in bf16, fp16 and f32 through
the single-operator entry points and checks, on EVERY element,
  * the bound, and that the output is finite;
  * a sentinel-filled output with guard rows: nothing written outside [B][HW][C] / [M][C], nothing left unwritten (the operator is
    called through the C ABI on a buffer the test owns);
  * a batch of N bit for bit equal to N single-image launches (GroupNorm), rows [0, m) of a launch equal to a launch of m rows
    (LayerNorm), and two runs bit-identical;
  * op_groupnorm_pre on hand-built gn_part values (the conv-made ones are in tests/test_gpu_gemm64.py).
No executor calls these kernels in place (unet.hip gn() -> t1 / t3, vae.hip gn() -> t1 / t3 / t, dit.hip lnmod() -> nb, each a
buffer of its own), so no in-place launch is tested.
The row-resident copies of the LayerNorm (csrc/rowres.hip) are isolated exactly: op_ln_linear with the 320 x 320 identity returns the
16-bit LayerNorm itself, op_ff_fused with ff_identity_weights() returns x + LN(x) (test_rowres_*_isolated).
test_launch_coverage holds the plans of the whole case list to the table of every reachable (form, NS, SILU, dtype) and
(form, CPL or MAXS, MOD, dtype), written from gn_plan / gn_onepass_slab / ln_plan of csrc/norm.hip, and prints the worst err / bound
per (form, dtype)."""
import time

import pytest
import torch

from tests import _norm64 as N

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
SENT = -12345.0              # fill of the output buffer: what the kernel must overwrite inside and leave alone outside
GUARD = 4                    # guard rows before and after the output


def _gn(HW, C0, C1=0, silu=1, eps=1e-5, B=2, groups=32, **kw):
    return dict(kind="gn", B=B, HW=HW, C0=C0, C1=C1, groups=groups, silu=silu, eps=eps, **kw)


def _ln(M, C=0, eps=1e-5, **kw):
    return dict(kind="ln", M=M, C=C, eps=eps, **kw)


# name -> problem.  GroupNorm: B, HW, C0, C1, groups, silu, eps, pre (statistics handed over as gn_part; 16-bit only).  LayerNorm: M,
# C or S (the width in 16-byte chunks: C = 8 S in the 16-bit types, 4 S in f32, for the arms that are chosen by S), eps, T (the
# modulated form, rows_per_batch = T).  fam: the input family (FAMILIES), "randn" by default.
CASES = {}
for _tag, (_s0, _s1, _s2, _s3) in (("512", (4096, 1024, 256, 64)), ("224", (784, 196, 49, 16))):
    # ---- SD1.5 / SDXL U-Net at 512 px (64 x 64 latents) and 224 px (28 x 28; odd sides 7, and 4 after the last stride-2 conv)
    for _hw, _c0, _c1, _silu in ((_s0, 320, 0, 1), (_s0, 320, 0, 0), (_s1, 320, 0, 1), (_s1, 640, 0, 1), (_s1, 640, 0, 0), (_s2, 640, 0, 1),
                                 (_s2, 1280, 0, 1), (_s2, 1280, 0, 0), (_s3, 1280, 0, 1), (_s3, 1280, 0, 0), (_s3, 1280, 1280, 1),
                                 (_s2, 1280, 1280, 1), (_s2, 1280, 640, 1), (_s1, 1280, 640, 1), (_s1, 640, 640, 1), (_s1, 640, 320, 1),
                                 (_s0, 640, 320, 1), (_s0, 320, 320, 1)):
        CASES[f"unet{_tag}_gn_{_hw}_{_c0}{'+' + str(_c1) if _c1 else ''}{'_silu' if _silu else ''}"] = \
            _gn(_hw, _c0, _c1, _silu, 1e-5 if _silu else 1e-6)
    for _m, _c in ((2 * _s0, 320), (2 * _s1, 640), (2 * _s2, 1280), (2 * _s3, 1280)):
        CASES[f"unet{_tag}_ln_{_m}_{_c}"] = _ln(_m, _c)
# ---- VAE encoder (one image): 512 px and 224 px maps, the mid-block attention's GroupNorm without SiLU; statistics from the conv
for _hw, _c in ((262144, 128), (65536, 128), (65536, 256), (16384, 256), (16384, 512), (4096, 512),
                (50176, 128), (12544, 128), (12544, 256), (3136, 256), (3136, 512), (784, 512)):
    CASES[f"vae_gn_{_hw}_{_c}_silu"] = _gn(_hw, _c, 0, 1, 1e-6, B=1)
CASES["vae_gn_4096_512"] = _gn(4096, 512, 0, 0, 1e-6, B=1)
CASES["vae_gn_784_512"] = _gn(784, 512, 0, 0, 1e-6, B=1)
CASES["vae_gn_4096_512_b3"] = _gn(4096, 512, 0, 0, 1e-6, B=3)
for _hw, _c in ((262144, 128), (65536, 256), (16384, 512), (4096, 512)):
    CASES[f"vae_gnpre_{_hw}_{_c}_silu"] = _gn(_hw, _c, 0, 1, 1e-6, B=1, pre=1)
# ---- DiT-XL/2 adaLN LayerNorm (hidden 1152): T = 256 and 196, odd and even image counts
for _t, _k in ((256, 2), (256, 3), (196, 2), (196, 5), (196, 8)):
    CASES[f"dit_lnmod_t{_t}_x{_k}"] = _ln(_t * _k, 1152, 1e-6, T=_t)
# ---- arms no production shape reaches.  GroupNorm: group counts 1 / 2 / 3 / 48 / 64 (folds wider than a wave, not a power of two,
# four threads per group), HW = 1 / 63 / 65 / 16385 (one row; below and above one 64-row slab; the 64-slab branch with ragged
# slabs), C at the GN_MAX_SLOTS limit (S0 = 1024 chunks: NS = 4), NS = 2, both without SiLU, pre with NS = 2 and 4
CASES.update({
    "gn_groups1": _gn(64, 1024, groups=1, silu=0), "gn_groups1_hw300": _gn(300, 256, groups=1),
    "gn_groups2": _gn(300, 64, groups=2, silu=0), "gn_groups2_concat": _gn(1024, 64, 64, groups=2),
    "gn_groups3": _gn(128, 96, groups=3, silu=0), "gn_groups3_hw1000": _gn(1000, 192, groups=3),
    "gn_groups48": _gn(1024, 384, groups=48, silu=0), "gn_groups48_small": _gn(16, 768, groups=48),
    "gn_groups64": _gn(2048, 512, groups=64), "gn_groups64_onepass": _gn(64, 2048, groups=64, silu=0),
    "gn_hw1": _gn(1, 1280, 1280), "gn_hw1_narrow": _gn(1, 64, silu=0, B=3),
    "gn_hw63": _gn(63, 320, silu=0), "gn_hw65": _gn(65, 320), "gn_hw65_concat": _gn(65, 640, 320, B=3),
    "gn_hw16385": _gn(16385, 64, B=1), "gn_hw16385_plain": _gn(16385, 128, 0, 0, 1e-6, B=2),
    "gn_maxslots": _gn(400, 0, S0=1024), "gn_maxslots_plain": _gn(400, 0, S0=1024, silu=0, B=1),
    "gn_maxslots_concat": _gn(200, 0, 0, S0=512, S1=512),
    "gn_ns2": _gn(1024, 0, S0=320), "gn_ns2_plain": _gn(300, 0, S0=320, S1=160, silu=0),
    "gn_pre_ns2": _gn(128, 0, S0=320, pre=1), "gn_pre_ns2_plain": _gn(64, 0, S0=320, pre=1, silu=0),
    "gn_pre_ns4": _gn(64, 0, S0=1024, pre=1, B=1), "gn_pre_ns4_plain": _gn(128, 0, S0=640, pre=1, silu=0, B=1),
    "gn_pre_plain": _gn(1024, 256, pre=1, silu=0, eps=1e-6), "gn_pre_groups8": _gn(256, 512, pre=1, groups=8),
    "gn_onepass_plain_concat": _gn(100, 640, 640, silu=0, B=3),
})
# LayerNorm: S = 7 k (CPL = 7: the wave-per-row arms without MOD, MAXS = 1), S = 72 / 100 (MAXS = 2), 160 (3), 200 / 384 (6: the
# widest row, C = 64 * 6 * VEC); lanes-per-row widths with LPR = 1 .. 64 and CPL = 1 / 3 / 5; row counts that reach 2 and 4 passes
for _s in (1, 2, 3, 5, 6, 8, 10, 12, 16, 20, 24, 32, 48, 64, 80, 7, 14, 56, 72, 100, 160, 200, 384):
    CASES[f"ln_s{_s}"] = _ln(133, S=_s)
CASES.update({"ln_s64_pass2": _ln(16400, S=64), "ln_s64_pass4": _ln(32800, S=64), "ln_s48_pass4": _ln(131100, S=48),
              "ln_s8_pass4": _ln(262200, S=8), "ln_s40_pass2": _ln(140001, S=40)})
# M = 1 and one below, at and one past a rows-per-workgroup multiple (4 waves x passes x 64 / LPR rows; 4 x RPW in the wave form)
for _s, _r in ((40, 32), (64, 4), (5, 256), (24, 32), (7, 32), (100, 8), (160, 8), (384, 4)):
    for _m in sorted({1, _r - 1, _r, _r + 1, 3 * _r - 1, 3 * _r, 3 * _r + 1}):
        CASES[f"ln_s{_s}_m{_m}"] = _ln(_m, S=_s)
# the modulated form on every wave-per-row arm (S = 40: MAXS 1, RPW 8, so 196 % RPW != 0 puts rows of both halves in one wave),
# and M not a multiple of T
for _s, _t, _m in ((40, 196, 980), (64, 49, 300), (128, 196, 588), (160, 7, 100), (192, 196, 392), (384, 196, 589), (144, 1, 37)):
    CASES[f"lnmod_s{_s}_t{_t}_m{_m}"] = _ln(_m, S=_s, eps=1e-6, T=_t)

# ---- input families beyond randn (see _inputs): name -> the cases they run on (base case, overrides)
FAMILIES = ("off4", "off32", "tiny", "const", "out1e3", "outmax", "neg")
_FAM_BASES = {
    "gn": ["unet512_gn_4096_320_silu", "unet512_gn_256_1280+640_silu", "unet512_gn_64_1280+1280_silu", "vae_gn_16384_512_silu",
           "vae_gn_4096_512", "vae_gnpre_4096_512_silu", "gn_groups3_hw1000", "gn_ns2"],
    "ln": ["unet512_ln_8192_320", "unet512_ln_512_1280", "dit_lnmod_t196_x5", "ln_s7", "ln_s100", "ln_s384"],
}
for _kind, _bases in _FAM_BASES.items():
    for _b in _bases:
        for _f in FAMILIES:
            if _f == "neg" and not CASES[_b].get("silu"):
                continue                                            # (large negative pre-activations matter where SiLU follows)
            if _f == "tiny":
                for _e in (1e-5, 1e-6):
                    CASES[f"{_b}|tiny_eps{_e:g}"] = dict(CASES[_b], fam="tiny", eps=_e)
            else:
                CASES[f"{_b}|{_f}"] = dict(CASES[_b], fam=_f)


def shape(name, dtype):
    """the case with its dtype-dependent widths resolved (S keys: 16-byte chunks)"""
    c = dict(CASES[name])
    V = N.vec(dtype)
    if c["kind"] == "gn":
        if "S0" in c:
            c["C0"], c["C1"] = c["S0"] * V, c.get("S1", 0) * V
    elif "S" in c:
        c["C"] = c["S"] * V
    return c


def _outmax(dtype):
    """the largest power of two of the compute dtype whose square still fits f32 (fp16: its largest finite value)"""
    return 65504.0 if dtype == torch.float16 else 2.0 ** 63


def inputs(name, dtype, device):
    """the seeded inputs of a case: dict(x0, x1, gamma, beta) for GroupNorm ([B][HW][C]), dict(x, gamma, beta) for LayerNorm
    (gamma / beta [2][C] in the modulated form).  Families: the statistics unit is a (image, group) or a row.
      randn   1.5 randn + 0.3
      off4 / off32  randn plus an offset of +-4 / +-32 per unit (|mean| / std about 4 / 32)
      tiny    1e-3 randn plus 2e-3 randn per unit: var about 1e-6, so eps (1e-5, 1e-6) is a first-order term
      const   unit 0 exactly constant (0.75), the whole second image / the second row exactly zero, randn elsewhere
      out1e3 / outmax  randn with one element per unit at 1e3 / at _outmax(dtype)
      neg     randn, beta = -200 on every other channel: SiLU's exp2 overflows to infinity there"""
    c = shape(name, dtype)
    fam = c.get("fam", "randn")
    g = torch.Generator().manual_seed(sum(map(ord, name.split("|")[0])) + 7 * len(fam))
    gn = c["kind"] == "gn"
    if gn:
        B, R, C, U = c["B"], c["HW"], c["C0"] + c["C1"], c["groups"]
    else:
        B, R, C, U = c["M"], 1, c["C"], 1
    x = torch.randn(B, R, U, C // U, generator=g)
    unit = lambda s=1.0: torch.randn(B, 1, U, 1, generator=g) * s
    if fam == "randn":
        x = 1.5 * x + 0.3
    elif fam in ("off4", "off32"):
        x = x + torch.sign(unit()) * float(fam[3:])
    elif fam == "tiny":
        x = 1e-3 * x + unit(2e-3)
    elif fam == "const":
        x[0, :, 0] = 0.75
        if B > 1:
            x[1] = 0.0
    elif fam in ("out1e3", "outmax"):
        x[:, R // 2, :, 1] = 1e3 if fam == "out1e3" else _outmax(dtype)
    x = x.reshape(B, R, C)
    mod = bool(c.get("T"))
    if mod:                                                         # scale2 / shift2 [2][C]: 1 + scale of either sign and size
        gamma = 0.5 * torch.randn(2 * C, generator=g)
    else:
        gamma = 1 + 0.1 * torch.randn(C, generator=g)
    beta = 0.1 * torch.randn((2 if mod else 1) * C, generator=g)
    if fam == "neg":
        beta[::2] = -200.0
    x = x.to(device).to(dtype)
    out = dict(gamma=gamma.to(device), beta=beta.to(device))
    if gn:
        out.update(x0=x[:, :, :c["C0"]].contiguous(), x1=x[:, :, c["C0"]:].contiguous() if c["C1"] else None)
    else:
        out["x"] = x.reshape(B, C)
    return c, out


def gn_part_of(x):
    """hand-built gn_part of x [B][HW][C]: f32 (sum, sum of squares) per 64 rows x 4-channel quad, from float64 sums"""
    B, HW, C = x.shape
    q = x.double().view(B, HW // 64, 64, C // 4, 4)
    return torch.stack([q.sum((2, 4)), (q * q).sum((2, 4))], -1).float().contiguous()


def plan_of(name, dtype):
    from diffsim_amd import engine
    c = shape(name, dtype)
    if c["kind"] == "gn":
        return engine.groupnorm_plan(c["C0"], c["C1"], c["B"], c["HW"], c["groups"], dtype, pre=bool(c.get("pre")))
    return engine.layernorm_plan(c["M"], c["C"], dtype, mod=bool(c.get("T")))


def runs():
    """(case, dtype) pairs: every case in every dtype, but the statistics-epilogue form in the 16-bit ones only"""
    return [(name, dt) for name, c in CASES.items() for dt in DT if not (c.get("pre") and dt == "f32")]


def ref_and_bound(c, t, dtype, plan):
    if c["kind"] == "gn":
        return N.gn_ref_and_bound(t["x0"], t["x1"], t["gamma"], t["beta"], c["groups"], c["eps"], c["silu"], dtype, N.gn_n_p(plan, c["HW"]))
    return N.ln_ref_and_bound(t["x"], t["gamma"], t["beta"], c["eps"], dtype, c.get("T", 0), depth=N.ln_depth(plan, dtype))


# (form, NS, SILU) and (form, CPL | MAXS, MOD) every dtype can reach; pre: the 16-bit types only (launch_groupnorm_pre)
_GN_ALL = [(f, ns, s) for f in ("twopass",) for ns in (1, 2, 4) for s in (0, 1)] + [("onepass", 1, s) for s in (0, 1)]
_GN_PRE = [("pre", ns, s) for ns in (1, 2, 4) for s in (0, 1)]
_LN_ALL = [("rows", cpl, 0) for cpl in (1, 3, 5)] + [("wave", m, mod) for m in (1, 2, 3, 6) for mod in (0, 1)]
REACHABLE = {dt: set(_GN_ALL + (_GN_PRE if dt != "f32" else []) + _LN_ALL) for dt in DT}


def plan_key(c, plan):
    if c["kind"] == "gn":
        return plan["form"], plan["NS"], int(bool(c["silu"]))
    return plan["form"], plan["CPL"] if plan["form"] == "rows" else plan["MAXS"], int(bool(c.get("T")))


WORST = {}                   # (case, dtype) -> largest err / bound (printed by test_launch_coverage)


def _eng():
    from diffsim_amd import engine
    return engine


def _launch(c, t, dtype, rows=None):
    """the operator through the C ABI on a sentinel-filled buffer with guard rows; returns the rows it wrote (a view).  rows: launch
    only the first `rows` images (GroupNorm) / rows (LayerNorm)."""
    from diffsim_amd import _lib
    from diffsim_amd.engine import _TORCH2DSIM
    L = _lib.lib()
    dt = _TORCH2DSIM[dtype]
    if c["kind"] == "gn":
        B, HW, C0, C1 = c["B"] if rows is None else rows, c["HW"], c["C0"], c["C1"]
        C, nrow = C0 + C1, (c["B"] if rows is None else rows) * c["HW"]
    else:
        C, nrow = c["C"], c["M"] if rows is None else rows
    buf = torch.full(((nrow + 2 * GUARD) * C,), SENT, dtype=dtype, device="cuda")
    out = buf[GUARD * C:(GUARD + nrow) * C]
    if c["kind"] == "gn" and c.get("pre"):
        part = t["part"][:B].contiguous()
        st = L.dsim_op_groupnorm_pre(t["x0"].data_ptr(), C, t["gamma"].data_ptr(), t["beta"].data_ptr(), out.data_ptr(), B, HW, c["groups"],
                                     float(c["eps"]), int(c["silu"]), dt, part.data_ptr(), HW // 64, None)
    elif c["kind"] == "gn":
        st = L.dsim_op_groupnorm(t["x0"].data_ptr(), C0, t["x1"].data_ptr() if C1 else None, C1, t["gamma"].data_ptr(), t["beta"].data_ptr(),
                                 out.data_ptr(), B, HW, c["groups"], float(c["eps"]), int(c["silu"]), dt, None)
    elif c.get("T"):
        st = L.dsim_op_layernorm_mod(t["x"].data_ptr(), t["gamma"].data_ptr(), t["beta"].data_ptr(), out.data_ptr(), nrow, C, c["T"],
                                     float(c["eps"]), dt, None)
    else:
        st = L.dsim_op_layernorm(t["x"].data_ptr(), t["gamma"].data_ptr(), t["beta"].data_ptr(), out.data_ptr(), nrow, C, float(c["eps"]), dt,
                                 None)
    _lib.check(st, "launch")
    torch.cuda.synchronize()
    sent = torch.tensor(SENT, dtype=dtype, device="cuda")
    assert (buf[:GUARD * C] == sent).all() and (buf[(GUARD + nrow) * C:] == sent).all(), "written outside the output"
    return out.view(nrow, C)


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


@pytest.mark.parametrize("name,dt", runs())
def test_norm_against_float64(name, dt):
    dtype = DT[dt]
    c, t = inputs(name, dtype, "cuda")
    plan = plan_of(name, dtype)
    if c.get("pre"):
        t["part"] = gn_part_of(t["x0"])
    got = _launch(c, t, dtype)
    sent = torch.tensor(SENT, dtype=dtype, device="cuda")
    assert not (got == sent).any(), "output elements left unwritten"
    ref, bound = ref_and_bound(c, t, dtype, plan)
    WORST[(name, dt)] = N.check(got, ref.view(got.shape), bound.view(got.shape), f"{name} {dt} {plan}")
    del ref, bound
    assert torch.equal(_bits(_launch(c, t, dtype)), _bits(got)), "two runs differ"
    if c["kind"] == "gn":
        HW = c["HW"]
        if c["B"] > 1:                                  # a batch of N = N single images, bit for bit
            for b in range(c["B"]):
                one = dict(t, x0=t["x0"][b:b + 1].contiguous(), x1=t["x1"][b:b + 1].contiguous() if c["C1"] else None)
                if c.get("pre"):
                    one["part"] = t["part"][b:b + 1]
                assert torch.equal(_bits(_launch(c, one, dtype, rows=1)), _bits(got[b * HW:(b + 1) * HW])), f"image {b} alone differs from the batch"
    else:
        m = max(1, c["M"] // 2 - 1)                     # rows [0, m) alone: every row is independent of the row count
        if m < c["M"]:
            assert torch.equal(_bits(_launch(c, t, dtype, rows=m)), _bits(got[:m])), f"the first {m} rows alone differ"


ROWRES_FAMS = ("randn", "off4", "off32", "tiny", "const", "out1e3")


def rowres_inputs(M, dtype, fam, device):
    name = f"rowres_{M}|{fam}"
    CASES[name] = dict(kind="ln", M=M, C=320, eps=1e-5, fam=fam)
    try:
        return inputs(name, dtype, device)[1]
    finally:
        del CASES[name]


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("M", [33, 96, 4128, 40000])
@pytest.mark.parametrize("fam", ROWRES_FAMS)
def test_rowres_layernorm_isolated(M, dt, fam):
    """rowres.hip's rowlin_kernel LayerNorm stage, alone: with w the 320 x 320 identity, out = LN(x) W^T is the 16-bit LayerNorm
    itself -- every product is with 1.0 or 0.0, the f32 sum of one value and zeros is exact, and storing a 16-bit value in its own
    type is exact -- so the output is held to the LayerNorm bound directly.  bf16, and the fp16 twin (f16::launch_rowlin)."""
    eng = _eng()
    dtype = DT[dt]
    t = rowres_inputs(M, dtype, fam, "cuda")
    eye = torch.eye(320, device="cuda")
    got = eng.op_ln_linear(t["x"], t["gamma"], t["beta"], eye, 1e-5)
    ref, bound = N.ln_ref_and_bound(t["x"], t["gamma"], t["beta"], 1e-5, dtype, depth=N.ln_depth(dict(form="rowres"), dtype))
    WORST[(f"rowres_lin_{M}|{fam}", dt)] = N.check(got, ref, bound, f"ln_linear identity M={M} {dt} {fam}")
    assert torch.equal(_bits(eng.op_ln_linear(t["x"], t["gamma"], t["beta"], eye, 1e-5)), _bits(got)), "two runs differ"


def ff_identity_weights(device):
    """w1, b1, w2, b2 with which op_ff_fused reduces to x + LN(x): h half = identity columns (h_j = LN(x)_j for j < 320, zero
    rows beyond), g half = zero weights with bias 8 -- gelu_fast(8) = 8 / (1 + 2^-39.8) = 8 exactly in f32 (its clamp u = 64) --
    so h * gelu(g) = 8 LN(x)_j, exact (a power of two), and w2 = 1/8 on the identity undoes it: the second GEMM returns LN(x)
    exactly in f32, b2 = 0, and the epilogue adds x: out = round16(x + LN16(x)), LN16 the kernel's 16-bit LayerNorm."""
    C = 320
    w1 = torch.zeros(8 * C, C, device=device)
    w1[:C] = torch.eye(C, device=device)
    b1 = torch.zeros(8 * C, device=device)
    b1[4 * C:] = 8.0
    w2 = torch.zeros(C, 4 * C, device=device)
    w2[:, :C] = torch.eye(C, device=device) / 8
    return w1, b1, w2, torch.zeros(C, device=device)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("M", [33, 96, 4128, 40000])
@pytest.mark.parametrize("fam", ["randn", "off32", "tiny", "const"])
def test_rowres_ff_layernorm_isolated(M, dt, fam):
    """ff_fused_kernel's LayerNorm stage through ff_identity_weights(): out = x + LN(x) up to the LayerNorm's own bound (which has
    its 16-bit rounding), gelu_fast's stated 2.6e-5 relative to 8 on a product that is then divided by 8 (|h| 2.6e-5 / 8 x 8), one
    f32 residual add and the output rounding."""
    eng = _eng()
    dtype = DT[dt]
    t = rowres_inputs(M, dtype, fam, "cuda")
    got = eng.op_ff_fused(t["x"], t["gamma"], t["beta"], *ff_identity_weights("cuda"), 1e-5)
    ln, lb = N.ln_ref_and_bound(t["x"], t["gamma"], t["beta"], 1e-5, dtype, depth=N.ln_depth(dict(form="rowres"), dtype))
    ref = t["x"].double() + ln
    u = N.U[dtype]
    E = lb + 2.6e-5 * ln.abs() + N.U32 * ref.abs()
    bound = u * ref.abs() + (1 + u) * E + (N.F16_FLOOR if dtype == torch.float16 else 0.0)
    WORST[(f"rowres_ff_{M}|{fam}", dt)] = N.check(got, ref, bound, f"ff_fused identity M={M} {dt} {fam}")


def test_launch_coverage():
    """The plans of the whole case list against REACHABLE, per dtype: an unreached entry fails.  Prints the worst err / bound per
    (form, dtype) of the cases that ran in this session."""
    t0 = time.time()
    seen = {dt: set() for dt in DT}
    forms = {}
    for name, dt in runs():
        c = shape(name, DT[dt])
        plan = plan_of(name, DT[dt])
        seen[dt].add(plan_key(c, plan))
        if (name, dt) in WORST:
            k = (("gn_" if c["kind"] == "gn" else ("lnmod_" if c.get("T") else "ln_")) + plan["form"], dt)
            forms[k] = max(forms.get(k, 0.0), WORST[(name, dt)])
    for (name, dt), w in WORST.items():
        if name.startswith("rowres_"):
            k = ("ln_" + name.split("|")[0].rsplit("_", 1)[0], dt)
            forms[k] = max(forms.get(k, 0.0), w)
    for dt in DT:
        assert seen[dt] == REACHABLE[dt], (dt, "missing", sorted(REACHABLE[dt] - seen[dt]), "unexpected", sorted(seen[dt] - REACHABLE[dt]))
    for k in sorted(forms):
        print(f"worst err/bound {k[1]:4s} {k[0]:16s} {forms[k]:.3f}")
    print(f"coverage pass {time.time() - t0:.1f} s")
