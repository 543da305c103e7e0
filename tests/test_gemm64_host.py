"""CPU checks of tests/_gemm64.py, the float64 GEMM reference and error bound the GPU GEMM tests hold the kernels to: the reference
agrees with torch's float64 F.linear / F.conv2d and with the oracle's modules (the VAE downsample, DiT's gated residual, the SDXL
resnet's per-half bias); the reference rounded to each dtype passes the bound, the same tensor with one element moved by 2 ulps does
not; and at production K the median bound stays within a few ulps of the output dtype, so that it cannot go slack unnoticed."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import _gemm64 as G
from oracle import cpu_ref as R

DT = [torch.float32, torch.bfloat16, torch.float16]


def _rand(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


@pytest.mark.parametrize("dtype", DT)
def test_linear_concat_and_wb_rows_match_torch(dtype):
    M, C0, C1, N = 96, 64, 32, 48
    a0, a1 = _rand(M, C0, seed=1).to(dtype), _rand(M, C1, seed=2).to(dtype)
    w, b = _rand(N, C0 + C1, seed=3), _rand(N, seed=4)
    ref = G.Gemm64(a0, w, dtype, a1=a1, bias=b).ref
    want = F.linear(torch.cat([a0, a1], 1).double(), w.to(dtype).double(), b.double())
    assert torch.allclose(ref, want, rtol=0, atol=1e-12)
    wb = _rand(3, N, C0, seed=5)
    ref = G.Gemm64(a0, wb, dtype, wb_rows=32).ref
    want = torch.cat([a0[i * 32:(i + 1) * 32].double() @ wb[i].to(dtype).double().T for i in range(3)])
    assert torch.allclose(ref, want, rtol=0, atol=1e-12)


@pytest.mark.parametrize("H,W,stride,ups,pad", [(7, 7, 1, 0, 1), (7, 5, 2, 0, 1), (14, 14, 2, 0, 1), (5, 6, 1, 1, 1), (8, 8, 2, 0, 0),
                                                (16, 12, 2, 0, 0)])
def test_conv_matches_torch_and_rows_subset(H, W, stride, ups, pad):
    B, C, N = 2, 16, 24
    x, w, b = _rand(B, H, W, C, seed=H + W), _rand(N, C, 3, 3, seed=7), _rand(N, seed=8)
    g = G.Gemm64(x, w, torch.float32, conv=dict(stride=stride, ups=ups, pad=pad), bias=b)
    xin = x.permute(0, 3, 1, 2).double()
    if ups:
        xin = F.interpolate(xin, scale_factor=2.0, mode="nearest")
    if pad:
        want = F.conv2d(xin, w.double(), b.double(), stride=stride, padding=1)
    else:
        want = F.conv2d(F.pad(xin, (0, 1, 0, 1)), w.double(), b.double(), stride=stride)
    want = want.permute(0, 2, 3, 1).reshape(-1, N)
    assert g.ref.shape == want.shape
    assert torch.allclose(g.ref, want, rtol=0, atol=1e-12)
    rows = G.row_subset(g.M, 16, boundaries=(g.M // B,), n_random=5)
    sub = G.Gemm64(x, w, torch.float32, conv=dict(stride=stride, ups=ups, pad=pad), bias=b, rows=rows)
    assert torch.equal(sub.ref, g.ref[rows])
    for t in range(0, g.M, 16):
        assert t in rows and min(t + 15, g.M - 1) in rows


def test_row_subset_has_tile_edges_and_boundaries():
    rows = G.row_subset(1000, 128, boundaries=(196, 392, 500), n_random=10, seed=3)
    for r in (0, 127, 128, 255, 895, 896, 999, 195, 196, 391, 392, 499, 500):
        assert r in rows
    assert torch.equal(rows, torch.unique(rows)) and int(rows.max()) < 1000


def test_vae_downsample_matches_the_oracle():
    m = R.VAEDownsample(16).double()
    with torch.no_grad():
        m.conv.weight.copy_(_rand(16, 16, 3, 3, seed=11))
        m.conv.bias.copy_(_rand(16, seed=12))
        x = _rand(2, 16, 10, 12, seed=13)
        want = m(x.double()).permute(0, 2, 3, 1).reshape(-1, 16)
    g = G.Gemm64(x.permute(0, 2, 3, 1).contiguous(), m.conv.weight.float(), torch.float32, conv=dict(stride=2, pad=0),
                 bias=m.conv.bias.float())
    assert torch.allclose(g.ref, want, rtol=0, atol=1e-12)


class _Const(torch.nn.Module):
    """stands in for a sub-module of the oracle block: returns a fixed tensor whatever its input"""

    def __init__(self, t):
        super().__init__()
        self.t = t

    def forward(self, *_):
        return self.t


def test_dit_gated_residual_and_mlp_match_the_oracle():
    """The oracle block's own forward (cpu_ref.py _DiTBlock) with its attention core fixed to o (so attn(...) = attn.proj(o)), the
    adaLN vectors given directly, and the MLP branch zeroed: x + gate_b * proj(o), gate_b the gate of batch element b (two CFG
    halves of T = 196 tokens).  And the block's Mlp with fc2 removed: fc1's tanh-GELU."""
    dim, T = 32, 196
    blk = R._DiTBlock(dim, 2, 4).double()
    with torch.no_grad():
        for p in blk.parameters():
            p.copy_(_rand(*p.shape, seed=p.numel()).double() * 0.2)
    o, x, gm = _rand(2, T, dim, seed=21), _rand(2, T, dim, seed=22), _rand(2, dim, seed=23)
    mods = _rand(2, 6 * dim, seed=24).double()
    mods[:, 2 * dim:3 * dim] = gm.double()                          # chunk 2 of adaLN_modulation(c): the attention gate
    proj = blk.attn.proj
    attn = _Const(proj(o.double()).detach())                         # proj of the fixed attention output
    blk.attn, blk.adaLN_modulation, mlp = attn, torch.nn.Identity(), blk.mlp
    blk.mlp = _Const(torch.zeros(2, T, dim, dtype=torch.float64))
    with torch.no_grad():
        want = blk(x.double(), mods).reshape(-1, dim)
    g = G.Gemm64(o.reshape(-1, dim), proj.weight.float(), torch.float32, bias=proj.bias.float(), gate=gm[0], gate2=gm[1],
                 rows_per_batch=T, residual=x.reshape(-1, dim))
    assert torch.allclose(g.ref, want, rtol=0, atol=1e-6)          # (the f64 module's weights are f32 values: exact)
    fc1 = mlp.fc1
    mlp.fc2 = torch.nn.Identity()
    with torch.no_grad():
        want = mlp(x.double()).reshape(-1, 4 * dim)
    g = G.Gemm64(x.reshape(-1, dim), fc1.weight.float(), torch.float32, bias=fc1.bias.float(), act=1)
    assert torch.allclose(g.ref, want, rtol=0, atol=1e-6)


def test_sdxl_resnet_per_half_bias_matches_the_oracle():
    """conv1 + time_emb_proj(silu(temb)) of a batch whose CFG halves alternate (elements 0, 2 uncond, 1, 3 cond): bias2 on the
    odd elements, rows_per_batch = H W"""
    cin, cout, tdim, H, W = 16, 32, 8, 7, 7
    rb = R.ResnetBlock2D(cin, cout, tdim, 4, 1e-5).double()
    with torch.no_grad():
        for p in rb.parameters():
            p.copy_(_rand(*p.shape, seed=p.numel() + 1).double() * 0.3)
    h0, temb2 = _rand(4, cin, H, W, seed=31), _rand(2, tdim, seed=32)
    temb = temb2[[0, 1, 0, 1]]
    with torch.no_grad():
        want = rb.conv1(h0.double()) + rb.time_emb_proj(F.silu(temb.double()))[:, :, None, None]
        tp = rb.time_emb_proj(F.silu(temb2.double())).float()
    want = want.permute(0, 2, 3, 1).reshape(-1, cout)
    b = rb.conv1.bias.float()
    g = G.Gemm64(h0.permute(0, 2, 3, 1).contiguous(), rb.conv1.weight.float(), torch.float32, conv=dict(), bias=b + tp[0],
                 bias2=b + tp[1], rows_per_batch=H * W)
    assert torch.allclose(g.ref, want, rtol=0, atol=1e-5)


def test_geglu_is_h_times_erf_gelu():
    M, K, C = 40, 64, 24
    x, w, b = _rand(M, K, seed=41), _rand(2 * C, K, seed=42) / 8, _rand(2 * C, seed=43)
    g = G.Gemm64(x, w, torch.float32, bias=b, epi="geglu")
    hg = F.linear(x.double(), w.double(), b.double())
    assert torch.allclose(g.ref, hg[:, :C] * F.gelu(hg[:, C:]), rtol=0, atol=1e-12)


def test_gelu_fast_error_constant():
    """the 2.6e-5 the bound charges the 16-bit GEGLU for (csrc/common.h gelu_fast) holds over the whole range"""
    x = torch.linspace(-20, 20, 400001, dtype=torch.float64)
    err = (G.gelu_fast64(x) - F.gelu(x)).abs().max().item()
    assert err <= G.GELU_FAST_ERR, err


def _cases(dtype, K):
    """(name, Gemm64) of every epilogue form at depth K, weights scaled as the models' (1 / sqrt(K))"""
    M, N = 64, 64
    x, w = _rand(M, K, seed=K), _rand(N, K, seed=K + 1) / math.sqrt(K)
    b, b2, gt, g2 = _rand(N, seed=1), _rand(N, seed=2), _rand(N, seed=3), _rand(N, seed=4)
    r = _rand(M, N, seed=5).to(dtype)
    kw = dict(bias=b)
    return [("plain", G.Gemm64(x.to(dtype), w, dtype, **kw)),
            ("bias2", G.Gemm64(x.to(dtype), w, dtype, bias2=b2, rows_per_batch=16, **kw)),
            ("residual", G.Gemm64(x.to(dtype), w, dtype, residual=r, **kw)),
            ("act", G.Gemm64(x.to(dtype), w, dtype, act=1, **kw)),
            ("gate", G.Gemm64(x.to(dtype), w, dtype, gate=gt, gate2=g2, rows_per_batch=16, residual=r, **kw)),
            ("geglu", G.Gemm64(x.to(dtype), w, dtype, epi="geglu", **kw))]


def _ulp(t, dtype):
    """the spacing of dtype at |t| (float64)"""
    e = torch.floor(torch.log2(t.abs().clamp_min(torch.finfo(dtype).tiny)))
    return torch.exp2(e) * torch.finfo(dtype).eps


@pytest.mark.parametrize("dtype", DT)
def test_rounded_reference_passes_and_two_ulps_fail(dtype):
    for name, g in _cases(dtype, 320):
        got = g.ref.to(dtype)
        assert g.check(got, name) <= 1.0
        if dtype == torch.float32:
            continue
        # move the largest element by 2 ulps of the output dtype: out of bound
        i = int(g.ref.abs().argmax())
        r, c = divmod(i, g.ref.shape[1])
        bad = got.double().clone()
        bad[r, c] += 2 * float(_ulp(bad[r, c], dtype))
        with pytest.raises(AssertionError):
            g.check(bad.to(dtype), name)


# median bound in ulps of the output at production K: the plain epilogue carries u_out (half an ulp) plus the accumulation term,
# lam u32 sqrt(K) s / |ref| ~ lam u32 K (random-sign data: s / |ref| ~ sqrt(K)); at K = 11520 that is 0.0055, i.e. 1.4 bf16 ulps
# and 11 fp16 ulps.  f32 outputs are dominated by the accumulation itself (the bound is then K-proportional: stated in u32 K).
MEDIAN_ULPS = {torch.bfloat16: 3.0, torch.float16: 16.0}


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("K", [1152, 2880, 11520])
def test_median_bound_stays_tight_at_production_k(dtype, K):
    g = G.Gemm64(_rand(256, K, seed=K).to(dtype), _rand(64, K, seed=K + 1) / math.sqrt(K), dtype, bias=_rand(64, seed=2) * 0.1)
    if dtype == torch.float32:
        med = float((g.bound / (g.ref.abs() * G.U32 * K)).median())
        assert med <= 16.0, med
    else:
        med = float((g.bound / _ulp(g.ref, dtype)).median())
        assert med <= MEDIAN_ULPS[dtype], med


def test_compiled_instantiations_are_the_coverage_tables():
    """Every gemm_kernel / gemm_skinny_kernel instantiation in the built library is in tests/test_gpu_gemm64.py's REACHABLE or
    UNREACHABLE table, and every entry of those tables is compiled: a new instantiation cannot go unlisted.  (Read from the
    library's mangled kernel-handle symbols; the small-batch kernel has no type parameter, so its bf16 / fp16 twins share names.)"""
    import re
    import shutil
    import subprocess
    from diffsim_amd import build
    from tests.test_gpu_gemm64 import REACHABLE, UNREACHABLE
    if shutil.which("nm") is None:
        pytest.skip("no nm")
    lib = build.build()
    syms = subprocess.run(["nm", lib], capture_output=True, text=True, check=True).stdout
    types = {"f": "f32", "DF16b": "bf16", "DF16_": "f16"}
    kinds = {0: "linear", 1: "conv3", 2: "conv3p"}
    eks = ("plain", "residual", "dit", "act", "plain_gn", "residual_gn")
    got = {dt: set() for dt in types.values()}
    for m in re.finditer(r"gemm_kernelI(f|DF16b|DF16_)((?:L[ib]\d+E){7})E", syms):
        bm, bn, mode, geglu, wm, wn, ek = (int(v) for v in re.findall(r"L[ib](\d+)E", m.group(2)))
        got[types[m.group(1)]].add((0, bm, bn, kinds[mode], geglu, eks[ek]))
    small = set()
    for m in re.finditer(r"gemm_skinny_kernelI((?:L[ib]\d+E){4})E", syms):
        mode, res, bm, bn = (int(v) for v in re.findall(r"L[ib](\d+)E", m.group(1)))
        small.add((1, bm, bn, kinds[mode], 0, eks[res]))
    assert got["f32"] and got["bf16"] and small, "no kernel symbols parsed"
    for dt in ("bf16", "f16"):
        got[dt] |= small
    want = {dt: REACHABLE[dt] | UNREACHABLE[dt] for dt in got}
    assert not any(REACHABLE[dt] & UNREACHABLE[dt] for dt in got)
    for dt in got:
        assert got[dt] == want[dt], (dt, "compiled, unlisted", sorted(got[dt] - want[dt]), "listed, not compiled", sorted(want[dt] - got[dt]))
