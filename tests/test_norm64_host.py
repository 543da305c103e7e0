"""CPU checks of tests/_norm64.py, the float64 reference and error bound the GPU norm tests hold the kernels to: the reference agrees
with the oracle's modules (oracle/cpu_ref.py: the resnet's GroupNorm + SiLU, the transformer's GroupNorm and LayerNorms, DiT's adaLN
modulation); the float32 replay of every kernel form stays inside the bound on every case of tests/test_gpu_norm64.py's table, input
families included -- the check that the chosen inputs keep the reference arithmetic alone inside the bound; the bound rejects what a
kernel bug would produce; it stays tight on the randn family; and the plans the library reports are the dispatch conditions of
csrc/norm.hip restated here, and reach every entry of the coverage table."""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import cpu_ref as R
from tests import _norm64 as N
from tests import test_gpu_norm64 as T

DT = T.DT


def _rand(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


# ---- the semantics are the models' ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("silu", [0, 1])
@pytest.mark.parametrize("groups,C0,C1", [(4, 32, 0), (4, 16, 16), (3, 24, 0), (8, 32, 64)])
def test_groupnorm_reference_matches_the_oracle(groups, C0, C1, silu):
    """The oracle resnet's norm1 (nn.GroupNorm) and its F.silu, in float64 on the concatenated NCHW map; without SiLU the
    transformer's GroupNorm (eps 1e-6)."""
    B, H, W, C = 2, 5, 7, C0 + C1
    eps = 1e-5 if silu else 1e-6
    x = _rand(B, H * W, C, seed=C + groups, scale=2.0) + 0.5
    if silu:
        m = R.ResnetBlock2D(C, C, 8, groups, eps).double().norm1
    else:
        m = R.Transformer2DModel(C, 1, 8, groups).double().norm
    assert m.eps == eps
    with torch.no_grad():
        m.weight.copy_(1 + 0.1 * _rand(C, seed=1))
        m.bias.copy_(0.1 * _rand(C, seed=2))
        want = m(x.double().permute(0, 2, 1).reshape(B, C, H, W))
        want = (F.silu(want) if silu else want).reshape(B, C, H * W).permute(0, 2, 1)
    ref, bound = N.gn_ref_and_bound(x[:, :, :C0], x[:, :, C0:] if C1 else None, m.weight.float(), m.bias.float(), groups, eps, silu,
                                    torch.float32, 4)
    assert torch.allclose(ref, want, rtol=0, atol=1e-6)         # (the f64 module's weights were rounded to f32 for the reference)
    assert (bound > 0).all()


def test_layernorm_reference_matches_the_oracle():
    blk = R.BasicTransformerBlock(64, 2, 16).double()
    x = _rand(37, 64, seed=3, scale=3.0) + 1
    with torch.no_grad():
        blk.norm3.weight.copy_(1 + 0.1 * _rand(64, seed=4))
        blk.norm3.bias.copy_(0.1 * _rand(64, seed=5))
        want = blk.norm3(x.double())
    ref, _ = N.ln_ref_and_bound(x, blk.norm3.weight.float(), blk.norm3.bias.float(), blk.norm3.eps, torch.float32)
    assert torch.allclose(ref, want, rtol=0, atol=1e-6)


class _Tap(torch.nn.Module):
    """stands in for the oracle block's attention: records its input (the modulated LayerNorm) and returns zeros"""

    def forward(self, x):
        self.seen = x
        return torch.zeros_like(x)


def test_modulated_layernorm_reference_matches_the_oracle():
    """The oracle DiT block's own forward with the adaLN vectors given directly: what reaches its attention is norm1(x) * (1 + scale_b)
    + shift_b, b the batch element -- the two CFG halves of T tokens each, which the kernel tells apart by (row // T) & 1."""
    dim, T_ = 32, 49
    blk = R._DiTBlock(dim, 2, 4).double()
    blk.attn, blk.adaLN_modulation = _Tap(), torch.nn.Identity()
    x = _rand(2, T_, dim, seed=6, scale=2.0)
    mods = _rand(2, 6 * dim, seed=7).double()
    with torch.no_grad():
        blk(x.double(), mods)
    shift, scale = mods[:, :dim].float(), mods[:, dim:2 * dim].float()        # chunk 0: shift_msa, chunk 1: scale_msa
    ref, _ = N.ln_ref_and_bound(x.reshape(-1, dim), scale.reshape(-1), shift.reshape(-1), 1e-6, torch.float32, rows_per_batch=T_)
    assert torch.allclose(ref, blk.attn.seen.reshape(-1, dim), rtol=0, atol=1e-6)
    # four images: halves alternate every T rows
    x4 = torch.cat([x, x]).reshape(-1, dim)
    ref4, _ = N.ln_ref_and_bound(x4, scale.reshape(-1), shift.reshape(-1), 1e-6, torch.float32, rows_per_batch=T_)
    assert torch.equal(ref4[:2 * T_], ref4[2 * T_:])


# ---- the dispatch, restated ---------------------------------------------------------------------------------------------------------
def py_onepass_slab(C0, C1, HW, groups, V):
    """gn_onepass_slab of csrc/norm.hip"""
    C, es = C0 + C1, 16 // V
    cpg, best, gs = C // groups, 0, 1
    while gs <= groups:
        CS = gs * cpg
        ok = not (groups % gs or CS % V or CS // V > 256)
        ok = ok and CS * es >= 256 and not (C1 and C0 % CS) and C // CS >= 2
        if ok:
            R_ = 256 // (CS // V)
            ok = -(-HW // R_) <= 24 and R_ * CS * 8 <= 48 * 1024
        if ok:
            best = CS
        gs *= 2
    return best


def py_gn_plan(C0, C1, B, HW, groups, dtype, pre):
    """gn_plan of csrc/norm.hip; None where it refuses"""
    V = N.vec(dtype)
    C = C0 + C1
    if B < 1 or HW < 1 or groups < 1 or C < V or C % groups or C0 % V or C1 % V or groups > 64 or C > 4 * 256 * V:
        return None
    if pre and (dtype == torch.float32 or C1 or (C // groups) % 4):
        return None
    CS = 0 if pre else py_onepass_slab(C0, C1, HW, groups, V)
    if CS:
        return dict(form="onepass", NS=1, UNR=0, CS=CS, tpr=CS // V, R=256 // (CS // V), chunks=0, rb=0)
    S = C // V
    tpr = min(S, 256)
    R_ = 256 // tpr
    if R_ * C * 8 > 64 * 1024:
        return None
    rb = max(1, min(64, HW // (R_ * 4), -(-1024 // B)))
    ns = -(-S // tpr)
    chunks = 64 if HW > 16384 else max(1, min(32, HW // 64))
    return dict(form="pre" if pre else "twopass", NS=1 if ns == 1 else (2 if ns == 2 else 4), UNR=4 if ns == 1 else (2 if ns == 2 else 1),
                CS=C, tpr=tpr, R=R_, chunks=1 if pre else chunks, rb=rb)


def py_ln_plan(M, C, dtype, mod):
    """ln_plan of csrc/norm.hip"""
    V = N.vec(dtype)
    if C < V or C % V or C > 64 * 6 * V or M < 1:
        return None
    S = C // V
    if not mod and S <= 80:
        LPR = 1
        while LPR < 64 and S % (LPR * 2) == 0:
            LPR *= 2
        if S // LPR in (1, 3, 5):
            rpw, passes = 64 // LPR, 4
            while passes > 1 and -(-M // (4 * passes * rpw)) < 2048:
                passes //= 2
            return dict(form="rows", LPR=LPR, CPL=S // LPR, passes=passes, MAXS=0, RPW=0, blocks=-(-M // (4 * passes * rpw)))
    maxs, rpw = (1, 8) if S <= 64 else ((2, 2) if S <= 128 else ((3, 2) if S <= 192 else (6, 1)))
    return dict(form="wave", LPR=0, CPL=0, passes=0, MAXS=maxs, RPW=rpw, blocks=-(-M // (4 * rpw)))


def test_plans_are_the_dispatch_conditions_and_cover_the_table():
    """engine.groupnorm_plan / layernorm_plan (the function the launchers call) against the conditions restated above, on every case
    and dtype; the case list reaches every entry of test_gpu_norm64.REACHABLE (the GPU file's test_launch_coverage, without a GPU)."""
    seen = {dt: set() for dt in DT}
    for name, dt in T.runs():
        c = T.shape(name, DT[dt])
        plan = T.plan_of(name, DT[dt])
        if c["kind"] == "gn":
            want = py_gn_plan(c["C0"], c["C1"], c["B"], c["HW"], c["groups"], DT[dt], bool(c.get("pre")))
        else:
            want = py_ln_plan(c["M"], c["C"], DT[dt], bool(c.get("T")))
        assert plan == want, (name, dt, plan, want)
        seen[dt].add(T.plan_key(c, plan))
    for dt in DT:
        assert seen[dt] == T.REACHABLE[dt], (dt, "missing", sorted(T.REACHABLE[dt] - seen[dt]), "unexpected", sorted(seen[dt] - T.REACHABLE[dt]))


def test_plans_refuse_what_the_launchers_refuse():
    from diffsim_amd import _lib, engine
    for args in ((320, 0, 2, 64, 33), (324, 0, 2, 64, 32), (320, 4, 2, 64, 4), (320, 0, 2, 64, 65), (16384, 0, 1, 64, 32), (320, 0, 0, 64, 32)):
        assert py_gn_plan(*args, torch.bfloat16, False) is None
        with pytest.raises(_lib.DsimError):
            engine.groupnorm_plan(*args, torch.bfloat16)
    with pytest.raises(_lib.DsimError):
        engine.groupnorm_plan(128, 0, 1, 4096, 32, torch.float32, pre=True)          # the statistics epilogue is 16-bit only
    with pytest.raises(_lib.DsimError):
        engine.groupnorm_plan(64, 64, 1, 4096, 32, torch.bfloat16, pre=True)
    for M, C in ((0, 320), (4, 324), (4, 3080), (4, 0)):
        assert py_ln_plan(M, C, torch.bfloat16, False) is None
        with pytest.raises(_lib.DsimError):
            engine.layernorm_plan(M, C, torch.bfloat16)
    assert engine.layernorm_plan(4, 3072, torch.bfloat16)["MAXS"] == 6 and engine.layernorm_plan(4, 1536, torch.float32, mod=True)["MAXS"] == 6


# ---- the reference arithmetic alone stays inside the bound -----------------------------------------------------------------------------
# (every case at full size, the VAE's 262144 x 128 maps included: a few seconds each on a CPU)
EMU_WORST = {}


@pytest.mark.parametrize("name,dt", T.runs())
def test_emulation_within_bound(name, dt):
    dtype = DT[dt]
    c, t = T.inputs(name, dtype, "cpu")
    plan = T.plan_of(name, dtype)
    ref, bound = T.ref_and_bound(c, t, dtype, plan)
    if c["kind"] == "gn":
        emu = N.emulate_groupnorm(t["x0"], t["x1"], t["gamma"], t["beta"], c["groups"], c["eps"], c["silu"], dtype, plan)
    else:
        emu = N.emulate_layernorm(t["x"], t["gamma"], t["beta"], c["eps"], dtype, plan, c.get("T", 0))
    EMU_WORST[(name, dt)] = N.check(emu, ref, bound, f"{name} {dt} {plan}")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("fam", T.ROWRES_FAMS)
def test_rowres_emulation_within_bound(dt, fam):
    t = T.rowres_inputs(96, DT[dt], fam, "cpu")
    ref, bound = N.ln_ref_and_bound(t["x"], t["gamma"], t["beta"], 1e-5, DT[dt], depth=N.ln_depth(dict(form="rowres"), DT[dt]))
    emu = N.emulate_layernorm(t["x"], t["gamma"], t["beta"], 1e-5, DT[dt], dict(form="rowres"))
    assert N.check(emu, ref, bound, f"rowres {dt} {fam}") <= 1.0


def test_ff_identity_weights_reduce_to_x_plus_layernorm():
    """the construction of test_gpu_norm64.test_rowres_ff_layernorm_isolated in float64, with the GEGLU of the oracle's FeedForward:
    x + ff(y) = x + y for the weights of ff_identity_weights(), and gelu_fast(8) = 8 in float32"""
    from tests._gemm64 import gelu_fast64
    w1, b1, w2, b2 = (v.double() for v in T.ff_identity_weights("cpu"))
    y = _rand(5, 320, seed=9).double()
    hg = y @ w1.T + b1
    h, g = hg.chunk(2, dim=-1)
    assert torch.allclose((h * F.gelu(g)) @ w2.T + b2, y, rtol=0, atol=1e-13)
    assert float(gelu_fast64(torch.tensor(8.0, dtype=torch.float64)).float()) == 8.0


# ---- the bound rejects what a kernel bug would produce -----------------------------------------------------------------------------
def _gn64(x, gamma, beta, groups, eps, silu, ddof=0, roll=0, stats=None):
    """GroupNorm in float64 with a bug switched on: variance over n - ddof; group boundaries `roll` channels off; stats: (mean, var)
    to apply instead of the tensor's own.  x [B][HW][C] float64.  Returns (y, (mean, var))."""
    B, HW, C = x.shape
    xs = torch.roll(x, -roll, 2) if roll else x
    v = xs.view(B, HW, groups, C // groups)
    mean = v.mean((1, 3), keepdim=True)
    var = ((v - mean) ** 2).sum((1, 3), keepdim=True) / (HW * (C // groups) - ddof)
    if stats is not None:
        mean, var = stats
    mean_c = mean.expand(B, 1, groups, C // groups).reshape(B, 1, C)
    var_c = var.expand(B, 1, groups, C // groups).reshape(B, 1, C)
    if roll:
        mean_c, var_c = torch.roll(mean_c, roll, 2), torch.roll(var_c, roll, 2)
    y = (x - mean_c) / torch.sqrt(var_c + eps) * gamma.double() + beta.double()
    return (F.silu(y) if silu else y), (mean, var)


def _gn_problem(name, dtype):
    c, t = T.inputs(name, dtype, "cpu")
    plan = T.plan_of(name, dtype)
    ref, bound = T.ref_and_bound(c, t, dtype, plan)
    x = (t["x0"] if t["x1"] is None else torch.cat([t["x0"], t["x1"]], 2)).double()
    return c, t, x, ref, bound


def _rejects(bad, ref, bound, dtype):
    return N.excess(bad.to(dtype), ref, bound) > 1.0


@pytest.mark.parametrize("dt", list(DT))
def test_bound_rejects_groupnorm_bugs(dt):
    dtype = DT[dt]
    # a correct result rounded to the dtype passes on each case used below
    for name in ("gn_hw1_narrow", "unet512_gn_256_1280+640_silu|off4", "unet512_gn_4096_320_silu|tiny_eps1e-06", "gn_hw65_concat"):
        c, t, x, ref, bound = _gn_problem(name, dtype)
        good, _ = _gn64(x, t["gamma"], t["beta"], c["groups"], c["eps"], c["silu"])
        assert N.excess(good.to(dtype), ref, bound) <= 1.0, name
    # variance over n - 1: visible in 16 bits only where a group is small (n = 2 here); at production group sizes (n >= 640) the
    # change, 1 / (2 n) relative, is below half a bf16 ulp and CANNOT be rejected in bf16 -- in f32 it is, at every size
    c, t, x, ref, bound = _gn_problem("gn_hw1_narrow", dtype)
    assert _rejects(_gn64(x, t["gamma"], t["beta"], c["groups"], c["eps"], c["silu"], ddof=1)[0], ref, bound, dtype)
    if dtype == torch.float32:
        c, t, x, ref, bound = _gn_problem("unet512_gn_256_1280+640_silu", dtype)
        assert _rejects(_gn64(x, t["gamma"], t["beta"], c["groups"], c["eps"], c["silu"], ddof=1)[0], ref, bound, dtype)
    # eps 1e-5 for 1e-6: the tiny-variance family (invisible elsewhere: at var = 2 it moves rstd by 2e-6 relative)
    c, t, x, ref, bound = _gn_problem("unet512_gn_4096_320_silu|tiny_eps1e-06", dtype)
    assert _rejects(_gn64(x, t["gamma"], t["beta"], c["groups"], 1e-5, c["silu"])[0], ref, bound, dtype)
    # on the per-group offset family: a group boundary one channel off; statistics of image b applied to image b + 1
    c, t, x, ref, bound = _gn_problem("unet512_gn_256_1280+640_silu|off4", dtype)
    g, b = t["gamma"], t["beta"]
    assert _rejects(_gn64(x, g, b, c["groups"], c["eps"], c["silu"], roll=1)[0], ref, bound, dtype)
    _, (mean, var) = _gn64(x, g, b, c["groups"], c["eps"], c["silu"])
    assert _rejects(_gn64(x, g, b, c["groups"], c["eps"], c["silu"], stats=(mean.roll(1, 0), var.roll(1, 0)))[0], ref, bound, dtype)
    # gamma / beta one 16-byte chunk off; SiLU dropped on one row; a row left at its sentinel; the second source at C0's stride
    V = N.vec(dtype)
    assert _rejects(_gn64(x, g.roll(V), b.roll(V), c["groups"], c["eps"], c["silu"])[0], ref, bound, dtype)
    good, _ = _gn64(x, g, b, c["groups"], c["eps"], c["silu"])
    plain, _ = _gn64(x, g, b, c["groups"], c["eps"], 0)
    bad = good.clone()
    bad[1, -1] = plain[1, -1]
    assert _rejects(bad, ref, bound, dtype)
    bad = good.clone()
    bad[0, -1] = T.SENT
    assert _rejects(bad, ref, bound, dtype)
    C0, C1 = c["C0"], c["C1"]
    flat = torch.cat([t["x1"].reshape(-1), torch.zeros(t["x1"].numel(), dtype=t["x1"].dtype)])
    idx = (torch.arange(c["B"] * c["HW"]) * C0).view(-1, 1) + torch.arange(C1).view(1, -1)
    xw = torch.cat([t["x0"], flat[idx].view(c["B"], c["HW"], C1)], 2).double()
    assert _rejects(_gn64(xw, g, b, c["groups"], c["eps"], c["silu"])[0], ref, bound, dtype)


def _ln64(x, gamma, beta, eps, ddof=0, half=None):
    C = x.shape[1]
    mean = x.mean(1, keepdim=True)
    var = ((x - mean) ** 2).sum(1, keepdim=True) / (C - ddof)
    xh = (x - mean) / torch.sqrt(var + eps)
    if half is None:
        return xh * gamma.double() + beta.double()
    return xh * (1 + gamma.double().view(2, C)[half]) + beta.double().view(2, C)[half]


@pytest.mark.parametrize("dt", list(DT))
def test_bound_rejects_layernorm_bugs(dt):
    dtype = DT[dt]
    V = N.vec(dtype)
    # variance over C - 1 (C = 8 V: 1 / (2 C) = 0.8 % .. 1.6 % of xhat, above a bf16 ulp; at C = 320 it is 0.16 %: below half a
    # bf16 ulp (0.2 %), rejected in fp16 and f32 only), gamma / beta a chunk off
    for name, ddof_ok in (("ln_s8", True), ("unet512_ln_8192_320", dtype != torch.bfloat16)):
        c, t = T.inputs(name, dtype, "cpu")
        ref, bound = T.ref_and_bound(c, t, dtype, T.plan_of(name, dtype))
        x = t["x"].double()
        assert N.excess(_ln64(x, t["gamma"], t["beta"], c["eps"]).to(dtype), ref, bound) <= 1.0
        if ddof_ok:
            assert _rejects(_ln64(x, t["gamma"], t["beta"], c["eps"], ddof=1), ref, bound, dtype), name
        assert _rejects(_ln64(x, t["gamma"].roll(V), t["beta"].roll(V), c["eps"]), ref, bound, dtype), name
    # eps 1e-5 for 1e-6 on the tiny-variance family
    name = "dit_lnmod_t196_x5|tiny_eps1e-06"
    c, t = T.inputs(name, dtype, "cpu")
    ref, bound = T.ref_and_bound(c, t, dtype, T.plan_of(name, dtype))
    half = (torch.arange(c["M"]) // c["T"]) & 1
    x = t["x"].double()
    assert N.excess(_ln64(x, t["gamma"], t["beta"], 1e-6, half=half).to(dtype), ref, bound) <= 1.0
    assert _rejects(_ln64(x, t["gamma"], t["beta"], 1e-5, half=half), ref, bound, dtype)
    # the MOD half taken from row & 1 instead of (row // T) & 1; one row of the tail left at its sentinel
    assert _rejects(_ln64(x, t["gamma"], t["beta"], 1e-6, half=torch.arange(c["M"]) & 1), ref, bound, dtype)
    bad = _ln64(x, t["gamma"], t["beta"], 1e-6, half=half)
    bad[-1] = T.SENT
    assert _rejects(bad, ref, bound, dtype)


def _ulp(t, dtype):
    e = torch.floor(torch.log2(t.abs().clamp_min(torch.finfo(dtype).tiny)))
    return torch.exp2(e) * torch.finfo(dtype).eps


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("name", ["unet512_gn_256_1280_silu", "vae_gn_4096_512", "unet512_ln_512_1280", "dit_lnmod_t196_x2"])
def test_rounded_reference_passes_and_two_ulps_fail(name, dt):
    """as tests/test_gemm64_host.py: in the 16-bit types the bound is within two ulps of the output.  In f32 two ulps (4 U32
    relative) are inside the accumulation terms (LAM U32 sqrt(n_p) and up): the bound CANNOT reject them there."""
    dtype = DT[dt]
    c, t = T.inputs(name, dtype, "cpu")
    ref, bound = T.ref_and_bound(c, t, dtype, T.plan_of(name, dtype))
    got = ref.to(dtype)
    assert N.excess(got, ref, bound) <= 1.0
    i = int(ref.abs().argmax())
    bad = got.double().reshape(-1).clone()
    bad[i] += 2 * float(_ulp(bad[i], dtype))
    assert N.excess(bad.reshape(ref.shape).to(dtype), ref, bound) > 1.0


# On the randn family the f32 terms are E / |ref| ~ LAM U32 sqrt(n) (1 / |xhat| + 0.55): the mean's error is absolute in xhat, the
# variance's proportional to it, and the median |xhat| of a normal sample is 0.67, so E ~ 2 LAM U32 sqrt(n) |ref| at the median; the
# affine and output roundings add a few U32.  16-bit: that is 1e-5 against u_out = 4e-3 / 5e-4, so the bound is the store's rounding.
@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("name", ["unet512_gn_4096_320", "unet512_gn_256_1280", "vae_gn_4096_512", "unet512_ln_8192_320", "unet512_ln_512_1280",
                                  "dit_lnmod_t256_x2"])
def test_median_bound_stays_tight_on_randn(name, dt):
    dtype = DT[dt]
    c, t = T.inputs(name, dtype, "cpu")
    plan = T.plan_of(name, dtype)
    ref, bound = T.ref_and_bound(c, t, dtype, plan)
    if dtype == torch.float32:
        n = N.gn_n_p(plan, c["HW"]) if c["kind"] == "gn" else N.ln_depth(plan, dtype)
        med = float((bound / (N.U32 * ref.abs())).median())
        assert med <= 4 * N.LAM * math.sqrt(n) + 16, (med, n)
    else:
        med = float((bound / (N.U[dtype] * ref.abs())).median())
        assert med <= 1.1, med


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_derived_bound_against_the_hand_set_one(dt):
    """tests/test_gpu_gemm64.py _check_gn keeps its hand-set u |ref| + 1e-5 (|ref| + 1) beside this module's bound, because the
    derived bound is NOT everywhere the smaller one on such inputs (a 128-channel map, statistics from 256-term partials): where
    silu(y) is near zero its absolute terms, LAM U32 sqrt(256) mean|x| / std and up, pass 1e-5.  Were this to stop holding, the
    hand-set bound could go."""
    dtype = DT[dt]
    x = (_rand(1, 4096, 128, seed=1) + 0.5 * _rand(1, 1, 128, seed=2)).to(dtype)
    gamma, beta = 1 + 0.1 * _rand(128, seed=3), 0.1 * _rand(128, seed=4)
    ref, bound = N.gn_ref_and_bound(x, None, gamma, beta, 32, 1e-6, True, dtype, 256)
    old = N.U[dtype] * ref.abs() + 1e-5 * (ref.abs() + 1.0)
    assert (bound > old).any() and (bound < old).any()
