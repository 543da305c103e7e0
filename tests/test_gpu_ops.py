"""Kernel-level parity: every HIP operator, called through the C ABI, against the same op in
plain torch fp32 on the CPU.  fp32 mode must agree to ~1e-5 (exact-f32 MFMA, different summation
order); the 16-bit modes (bf16, fp16) are compared on inputs rounded to the compute dtype with a tolerance sized to it."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]


def _tol(dtype):
    # bf16: 8 significant bits; fp16 (the reference drivers' dtype): 11
    return (2e-5, 2e-5) if dtype == torch.float32 else ((2e-2, 2e-2) if dtype == torch.bfloat16 else (3e-3, 3e-3))


def _dev(t, dtype=None):
    t = t.cuda()
    return t.to(dtype).contiguous() if dtype is not None else t.contiguous()


def _q(t, dtype):
    """round-trip through the compute dtype so the CPU reference sees the same operand values"""
    return t.to(dtype).float()


def _close(got, want, dtype, scale=None):
    rt, at = _tol(dtype)
    got = got.float().cpu()
    s = float(want.abs().max()) if scale is None else scale
    err = (got - want).abs().max().item()
    assert err <= at * max(s, 1e-6) + 1e-7, f"max err {err:.3e} vs scale {s:.3e}"
    assert torch.isfinite(got).all()


def _f64(got, a0, w, dtype, **kw):
    """beside _close: every element within tests/_gemm64.py's float64 bound (a0 the CPU operand, w / bias the f32 values)"""
    from tests import _gemm64 as G
    G.Gemm64(a0.to(dtype), w, dtype, **kw).check(got.float().cpu().reshape(-1, got.shape[-1]), "float64 bound")


def _attn_f64(got, q, k, v, H, dtype, fp8=False):
    """beside _close: every element within tests/_attn64.py's float64 bound for the kernel dsim_attention_plan names (q [B][Nq][H D],
    k / v [Bkv][Nk][H D] CPU float32 values; above 2^22 query-key pairs per head, test_gpu_attn64's row subset)"""
    from diffsim_amd import engine
    from tests import _attn64 as A
    from tests.test_gpu_attn64 import rows_checked
    B, Nq, HD = q.shape
    Bkv, Nk = k.shape[:2]
    D = HD // H
    tdt = torch.bfloat16 if fp8 else dtype
    kind = engine.attention_plan(B, Bkv, H, Nq, Nk, D, tdt, fp8=fp8)
    rows = rows_checked(Nq, Nk)
    qh = A.heads(_q(q, tdt).double()[:, rows].cuda(), B, len(rows), H, D)
    kh, vh = (A.expand_kv(A.heads(_q(t, tdt).double().cuda(), Bkv, Nk, H, D), B, Bkv, H) for t in (k, v))
    ref, bound = A.ref_and_bound(qh, kh, vh, A.Spec(kind, tdt, D))
    r = A.excess(A.heads(got.double().cuda()[:, rows], B, len(rows), H, D), ref, bound)
    assert r <= 1.0, f"{kind} d{D}: err / bound {r:.3f}"


def _norm_f64(got, x0, x1, gamma, beta, dtype, *, groups=0, eps=1e-5, silu=False):
    """beside _close: every element within tests/_norm64.py's float64 bound for the form engine.groupnorm_plan / layernorm_plan names
    (x0 / x1 the device operands in the compute dtype; groups = 0: LayerNorm of x0 [M][C])"""
    from diffsim_amd import engine
    from tests import _norm64 as N
    if groups:
        B, HW, C0 = x0.shape
        plan = engine.groupnorm_plan(C0, 0 if x1 is None else x1.shape[2], B, HW, groups, dtype)
        ref, bound = N.gn_ref_and_bound(x0, x1, gamma.cuda(), beta.cuda(), groups, eps, silu, dtype, N.gn_n_p(plan, HW))
    else:
        plan = engine.layernorm_plan(x0.shape[0], x0.shape[1], dtype)
        ref, bound = N.ln_ref_and_bound(x0, gamma.cuda(), beta.cuda(), eps, dtype, depth=N.ln_depth(plan, dtype))
    N.check(got, ref, bound, f"float64 bound {plan}")


def _rowres_f64(eng, got, x, lg, lb, dtype, *, w=None, ff=None):
    """beside _close: the row-resident kernels within tests/_rowres64.py's float64 bounds (x the device operand in the compute dtype,
    the rest CPU f32 values).  w: op_ln_linear, staged -- with the 320 x 320 identity the kernel returns its own 16-bit LayerNorm
    (lg None: x itself), and the dense launch is the plain GEMM epilogue on that operand; ff = (w1, b1, w2, b2): op_ff_fused against
    the chained bound.  Above 4096 rows, test_gpu_rowres64's row subsets."""
    from tests import _gemm64 as G
    from tests import _norm64 as N
    from tests import _rowres64 as R
    M = x.shape[0]
    if ff is None:
        from tests.test_gpu_rowres64 import lin_rows
        operand = x if lg is None else eng.op_ln_linear(x, _dev(lg), _dev(lb), torch.eye(R.C, device="cuda"), 1e-5)
        rows = lin_rows(M)
        G.Gemm64(operand, w.cuda(), dtype, rows=rows).check(got if rows is None else got[rows.cuda()], "float64 bound, staged")
    else:
        rows = None if M <= 4096 else G.row_subset(M, 128)
        ref, bound = R.ff_ref_and_bound(x, *(_dev(t) for t in (lg, lb) + tuple(ff)), 1e-5, dtype, rows=rows)
        N.check(got if rows is None else got[rows.cuda()], ref, bound, "float64 bound, chained")


def _h16_cases(cases):
    """every case in bf16 under the id it had before the fp16 twins were tested, and again in fp16"""
    out = []
    for c in cases:
        c = c if isinstance(c, tuple) else (c,)
        name = "-".join(str(v) for v in c)
        out += [pytest.param(*c, torch.bfloat16, id=name), pytest.param(*c, torch.float16, id=name + "-fp16")]
    return out


@pytest.fixture(scope="module")
def eng():
    from diffsim_amd import engine
    return engine


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,N,K", [(300, 320, 320), (256, 1280, 2560), (154, 640, 768), (64, 64, 128),
                                   (1000, 1920, 640), (4096, 160, 64)])
def test_linear(eng, dtype, M, N, K):
    g = torch.Generator().manual_seed(M + N + K)
    x = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) / math.sqrt(K)
    b = torch.randn(N, generator=g)
    r = torch.randn(M, N, generator=g)
    want = F.linear(_q(x, dtype), _q(w, dtype), b)
    got = eng.op_linear(_dev(x, dtype), _dev(w), _dev(b))
    _close(got, want, dtype)
    _f64(got, x, w, dtype, bias=b)
    want2 = want - b + _q(r, dtype)
    got2 = eng.op_linear(_dev(x, dtype), _dev(w), None, _dev(r, dtype))
    _close(got2, want2, dtype)
    _f64(got2, x, w, dtype, residual=r.to(dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,C", [(256, 320), (130, 64), (512, 1280), (4100, 640)])   # 32-row blocks; 16-row blocks on 128x160 and 256x320 tiles
def test_linear_geglu(eng, dtype, M, C):
    g = torch.Generator().manual_seed(M + C)
    x = torch.randn(M, C, generator=g)
    w = torch.randn(8 * C, C, generator=g) / math.sqrt(C)
    b = torch.randn(8 * C, generator=g)
    hg = F.linear(_q(x, dtype), _q(w, dtype), b)
    hh, gg = hg.chunk(2, dim=-1)
    want = hh * F.gelu(gg)
    got = eng.op_linear(_dev(x, dtype), _dev(w), _dev(b), None, geglu=True)
    assert got.shape == (M, 4 * C)
    _close(got, want, dtype)
    _f64(got, x, w, dtype, bias=b, epi="geglu")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,H,W,Cin,Cout,stride,ups", [
    (2, 16, 16, 64, 128, 1, False), (3, 8, 8, 320, 320, 1, False), (2, 16, 16, 128, 128, 2, False),
    (2, 8, 8, 128, 64, 1, True), (1, 5, 7, 64, 160, 1, False), (2, 32, 32, 320, 320, 1, False),
    (2, 8, 8, 1920, 1280, 1, False), (2, 6, 6, 64, 64, 2, False),
    (2, 7, 7, 64, 128, 2, False), (1, 9, 5, 128, 64, 2, False)])          # odd sides through stride 2: ceil(H / 2) rows (--image_size 224)
def test_conv3x3(eng, dtype, B, H, W, Cin, Cout, stride, ups):
    g = torch.Generator().manual_seed(B * 1000 + H + Cin + Cout + stride)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin)
    b = torch.randn(Cout, generator=g)
    xin = _q(x, dtype)
    if ups:
        xin = F.interpolate(xin, scale_factor=2.0, mode="nearest")
    want = F.conv2d(xin, _q(w, dtype), b, stride=stride, padding=1)          # NCHW
    r = torch.randn(want.shape, generator=g)
    got = eng.op_conv3x3(_dev(x.permute(0, 2, 3, 1), dtype), _dev(w), _dev(b), None, stride, ups)
    _close(got.float().cpu().permute(0, 3, 1, 2), want, dtype)
    cv = dict(stride=stride, ups=int(ups))
    _f64(got, x.permute(0, 2, 3, 1).contiguous(), w, dtype, conv=cv, bias=b)
    got2 = eng.op_conv3x3(_dev(x.permute(0, 2, 3, 1), dtype), _dev(w), _dev(b), _dev(r.permute(0, 2, 3, 1), dtype),
                          stride, ups)
    _close(got2.float().cpu().permute(0, 3, 1, 2), want + _q(r, dtype), dtype)
    _f64(got2, x.permute(0, 2, 3, 1).contiguous(), w, dtype, conv=cv, bias=b, residual=r.permute(0, 2, 3, 1).to(dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,HW,C0,C1,silu,eps", [
    (2, 256, 320, 0, True, 1e-5), (3, 64, 1280, 640, True, 1e-5), (2, 4096, 320, 0, False, 1e-6),
    (2, 16, 256, 128, True, 1e-5), (1, 1, 1280, 1280, True, 1e-5), (2, 1024, 64, 0, True, 1e-5),
    (2, 40000, 128, 0, True, 1e-6),         # a VAE-sized map: 64 statistics slabs per image, ragged slab lengths
    # the one-pass form (register-resident slabs of whole groups) at the 16 x 16 / 8 x 8 level shapes: single source,
    # both concat widths (2560 = one-pass, 1920 = 60-channel groups straddle 16-byte chunks -> two-pass), wide batch
    (3, 256, 1280, 0, True, 1e-5), (2, 256, 1280, 1280, True, 1e-5), (2, 256, 1280, 640, True, 1e-5),
    (2, 64, 1280, 1280, True, 1e-5), (5, 64, 1280, 0, False, 1e-6), (2, 256, 640, 0, True, 1e-5),
    (130, 64, 1280, 0, True, 1e-5), (2, 100, 320, 0, True, 1e-5), (2, 576, 1280, 0, True, 1e-5)])
def test_groupnorm(eng, dtype, B, HW, C0, C1, silu, eps):
    g = torch.Generator().manual_seed(HW + C0 + C1)
    C = C0 + C1
    x = torch.randn(B, HW, C, generator=g) * 2.0 + 0.7
    gamma = 1 + 0.1 * torch.randn(C, generator=g)
    beta = 0.1 * torch.randn(C, generator=g)
    xq = _q(x, dtype)
    want = F.group_norm(xq.permute(0, 2, 1), 32, gamma, beta, eps)
    if silu:
        want = F.silu(want)
    want = want.permute(0, 2, 1)
    x0 = _dev(x[:, :, :C0], dtype)
    x1 = _dev(x[:, :, C0:], dtype) if C1 else None
    got = eng.op_groupnorm(x0, x1, _dev(gamma), _dev(beta), 32, eps, silu)
    _close(got, want, dtype)
    _norm_f64(got, x0, x1, gamma, beta, dtype, groups=32, eps=eps, silu=silu)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,HW,C,groups", [(2, 300, 64, 2), (3, 128, 96, 3), (2, 256, 512, 8), (2, 64, 1024, 1), (2, 1024, 384, 48)])
def test_groupnorm_group_counts(eng, dtype, B, HW, C, groups):
    """Group counts other than 32: the statistics folds split 256 threads over the groups (a group wider than a wave, a
    count that is not a power of two, one group, more groups than a wave has quarter-rows)."""
    g = torch.Generator().manual_seed(HW + C + groups)
    x = torch.randn(B, HW, C, generator=g) * 1.5 - 0.4
    gamma = 1 + 0.1 * torch.randn(C, generator=g)
    beta = 0.1 * torch.randn(C, generator=g)
    want = F.group_norm(_q(x, dtype).permute(0, 2, 1), groups, gamma, beta, 1e-5).permute(0, 2, 1)
    got = eng.op_groupnorm(_dev(x, dtype), None, _dev(gamma), _dev(beta), groups, 1e-5, False)
    _close(got, want, dtype)
    _norm_f64(got, _dev(x, dtype), None, gamma, beta, dtype, groups=groups)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,C", [
    (257, 320), (64, 1280), (100, 64), (33, 640),
    # the lanes-per-row form (rows up to 80 16-byte chunks): 1 / 3 / 5 chunks per lane, 4 .. 64 lanes per row, ragged row counts,
    # and row counts large enough for 2 and 4 passes per wave
    (1000, 192), (77, 96), (513, 160), (130, 256), (65, 512), (140001, 320), (262200, 64)])
def test_layernorm(eng, dtype, M, C):
    g = torch.Generator().manual_seed(M + C)
    x = torch.randn(M, C, generator=g) * 3 + 1
    gamma = 1 + 0.1 * torch.randn(C, generator=g)
    beta = 0.1 * torch.randn(C, generator=g)
    want = F.layer_norm(_q(x, dtype), (C,), gamma, beta, 1e-5)
    got = eng.op_layernorm(_dev(x, dtype), _dev(gamma), _dev(beta))
    _close(got, want, dtype)
    _norm_f64(got, _dev(x, dtype), None, gamma, beta, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,Bkv,H,Nq,Nk,D", [
    (2, 2, 8, 256, 256, 160), (2, 2, 8, 1024, 1024, 80), (2, 2, 8, 4096, 4096, 40), (4, 2, 8, 256, 77, 160),
    (2, 2, 4, 64, 64, 16), (2, 2, 4, 16, 13, 64), (3, 3, 2, 100, 70, 32), (2, 2, 8, 64, 64, 160), (2, 1, 16, 256, 256, 72),
    # ragged key counts around the 32-key MFMA blocks and the 64-key tiles for every production head dim, the 77-key
    # cross-attention shapes, a single tile, many tiles
    (2, 2, 8, 300, 77, 40), (4, 2, 5, 200, 77, 64), (2, 2, 4, 130, 200, 72), (2, 2, 4, 96, 31, 80), (2, 2, 2, 64, 33, 40),
    (2, 1, 2, 64, 64, 40), (2, 2, 2, 128, 65, 64), (1, 1, 2, 160, 97, 40), (2, 2, 2, 96, 129, 80), (1, 1, 3, 64, 449, 72),
    # the short-key kernel (bf16, <= 96 keys, d = 40 / 80) with several query blocks per workgroup and a ragged last block
    (16, 2, 8, 4096 + 40, 77, 40), (32, 2, 8, 1024 + 7, 77, 80), (2, 2, 8, 512, 96, 40),
    # the pipelined long-key kernel (bf16, d = 40, keys a multiple of 64 and >= 2048) with a ragged last query block
    (1, 1, 2, 300, 2112, 40), (2, 1, 3, 257, 2048, 40),
    # two query blocks per wave sharing the fragment reads (16-bit, d = 64, >= 256 queries, > 96 keys): running-maximum and
    # fixed-reference (>= 1024 keys) forms, ragged last query block, ragged last key tile, K / V shared between batch elements
    (2, 2, 3, 256, 200, 64), (2, 1, 2, 300, 1024, 64), (1, 1, 2, 513, 1100, 64), (2, 2, 10, 1024, 1024, 64)])
def test_attention(eng, dtype, B, Bkv, H, Nq, Nk, D):
    g = torch.Generator().manual_seed(Nq + Nk + D)
    q = torch.randn(B, Nq, H * D, generator=g) * 1.3
    k = torch.randn(Bkv, Nk, H * D, generator=g) * 1.3
    v = torch.randn(Bkv, Nk, H * D, generator=g)
    qq, kq, vq = _q(q, dtype), _q(k, dtype), _q(v, dtype)
    idx = torch.arange(B) % Bkv
    want = F.scaled_dot_product_attention(qq.view(B, Nq, H, D).transpose(1, 2),
                                          kq[idx].view(B, Nk, H, D).transpose(1, 2),
                                          vq[idx].view(B, Nk, H, D).transpose(1, 2))
    want = want.transpose(1, 2).reshape(B, Nq, H * D)
    got = eng.op_attention(_dev(q, dtype), _dev(k, dtype), _dev(v, dtype), H)
    _close(got, want, dtype)
    _attn_f64(got, q, k, v, H, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_pair_score_against_golden_tail(eng, dtype, golden_dir):
    """Seeded q/k/v sets whose scores were produced by the REFERENCE's DiffSim.diffsim tail
    (tests/golden/g4_tail.npz): cosine and mse, several shapes, A == B."""
    import os
    g4 = np.load(os.path.join(golden_dir, "g4_tail.npz"))
    for i in range(10):
        shp = tuple(int(x) for x in g4[f"shape_{i}"])
        gen = torch.Generator("cpu").manual_seed(int(g4[f"seed_{i}"][0]))
        sets = [[torch.randn(shp, generator=gen) * (1.5 if j == 0 else 1.0) for j in range(3)] for _ in range(2)]
        mixw = 0.3 + 0.07 * i
        sets[1] = [mixw * a + (1 - mixw) * b for a, b in zip(sets[0], sets[1])]
        if i == 8:
            sets[1] = [t.clone() for t in sets[0]]
        Bc, H, N, D = shp
        # (B,H,N,D) -> engine layout [img][B][N][H*D]
        feats = [torch.stack([s[j].transpose(1, 2).reshape(Bc, N, H * D) for s in sets]) for j in range(3)]
        q, k, v = (_dev(f, dtype) for f in feats)
        ia = torch.tensor([0], dtype=torch.int32).cuda()
        ib = torch.tensor([1], dtype=torch.int32).cuda()
        for sim in ("cosine", "mse"):
            got = eng.pair_score(q, k, v, ia, ib, H, sim).cpu()
            want = float(g4[f"score_{i}_{sim}"][0])
            tol = 1e-4 if dtype == torch.float32 else 3e-2
            assert abs(float(got[0]) - want) <= tol * max(abs(want), 1e-2), (i, sim, float(got[0]), want)


def test_pair_score_batched_indices_and_determinism(eng):
    g = torch.Generator().manual_seed(5)
    nf, B, H, N, D = 5, 2, 8, 256, 160
    q, k, v = (torch.randn(nf, B, N, H * D, generator=g).cuda() for _ in range(3))
    ia = torch.tensor([0, 0, 3, 4, 2], dtype=torch.int32).cuda()
    ib = torch.tensor([1, 2, 3, 0, 1], dtype=torch.int32).cuda()
    s1 = eng.pair_score(q, k, v, ia, ib, H, "cosine")
    s2 = eng.pair_score(q, k, v, ia, ib, H, "cosine")
    assert torch.equal(s1, s2)                       # fixed-order reduction: bit-reproducible
    assert abs(float(s1[2]) - 1.0) < 1e-5            # image vs itself with identical features
    for p in range(5):                               # batch-of-N == N singles, bit for bit
        sp = eng.pair_score(q, k, v, ia[p:p + 1].clone(), ib[p:p + 1].clone(), H, "cosine")
        assert torch.equal(sp[0], s1[p])
    # linearity-style property: swapping roles leaves the symmetric score unchanged
    s3 = eng.pair_score(q, k, v, ib, ia, H, "cosine")
    assert torch.allclose(s1, s3, atol=1e-6)


# ---- persistent GEMM: more tiles than resident workgroups, ragged last row tile --------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,N,K,res", [(256 * 530 + 77, 320, 320, True),      # 256x320 tiles (bf16), 531 tiles > 256 WGs
                                       (128 * 1100 + 5, 160, 64, False),      # 128x160 tiles, 1101 tiles > 512 WGs
                                       (256 * 300 + 1, 512, 128, True),       # 256x256 tiles, 2 column tiles
                                       (256 * 280 + 9, 1152, 128, True),      # 256x192 tiles (DiT widths), 6 column tiles
                                       (256 * 260, 384, 192, False),         # 256x192, plain epilogue
                                       (256 * 40 + 3, 3456, 128, True)])      # DiT qkv width: 256x256 tiles, ragged 14th column tile
def test_linear_many_tiles_per_workgroup(eng, dtype, M, N, K, res):
    """Each persistent workgroup walks several tiles (stage prefetch under the epilogue, LDS buffer parity carried
    across tiles, ragged last tile): every row of the output is checked against torch on a strided sample plus the
    whole ragged tail."""
    g = torch.Generator().manual_seed(N + K)
    x = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) / math.sqrt(K)
    b = torch.randn(N, generator=g)
    r = torch.randn(M, N, generator=g) if res else None
    got = eng.op_linear(_dev(x, dtype), _dev(w), _dev(b), _dev(r, dtype) if res else None).float().cpu()
    rows = torch.cat([torch.arange(0, M, 97), torch.arange(M - 300, M)])
    want = F.linear(_q(x[rows], dtype), _q(w, dtype), b) + (_q(r[rows], dtype) if res else 0)
    _close(got[rows], want, dtype)
    assert torch.isfinite(got).all()
    from tests import _gemm64 as G
    G.Gemm64(x.to(dtype), w, dtype, bias=b, residual=r.to(dtype) if res else None, rows=rows).check(got[rows], "float64 bound")


@pytest.mark.parametrize("dtype", DTYPES)
def test_conv3x3_many_tiles_per_workgroup(eng, dtype):
    """3x3 conv, 64 -> 320 channels at 64x64, 20 images: 320 row tiles of 256 (bf16) / 640 of 128 (f32) per column tile."""
    B, H, W, Cin, Cout = 20, 64, 64, 64, 320
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, H, W, Cin, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin)
    b = torch.randn(Cout, generator=g)
    r = torch.randn(B, H, W, Cout, generator=g)
    got = eng.op_conv3x3(_dev(x, dtype), _dev(w), _dev(b), _dev(r, dtype)).float().cpu()
    sel = [0, 7, 19]
    want = F.conv2d(_q(x[sel], dtype).permute(0, 3, 1, 2), _q(w, dtype), b, padding=1).permute(0, 2, 3, 1) + _q(r[sel], dtype)
    _close(got[sel], want, dtype)
    assert torch.isfinite(got).all()
    _f64(got[sel], x[sel], w, dtype, conv={}, bias=b, residual=r[sel].to(dtype))


# ---- fp8 (e4m3) MFMA attention: the DiT mode of BASELINE config 5 ---------------------------------------------------
@pytest.mark.parametrize("B,Bkv,H,Nq,Nk,D", [(3, 3, 16, 256, 256, 72), (2, 2, 4, 64, 64, 32), (2, 1, 4, 200, 77, 72)])
def test_attention_fp8(eng, B, Bkv, H, Nq, Nk, D):
    """Both matmuls in e4m3 (3 mantissa bits): compared with fp32 SDPA on the bf16-rounded inputs under an fp8-sized,
    stated tolerance -- max error 12 % of the output range (measured 5-8 %), mean error 1.5 % (measured 0.6 %); and
    against the bf16 kernel."""
    g = torch.Generator().manual_seed(B + Nq + D)
    q = torch.randn(B, Nq, H * D, generator=g) * 0.9
    k = torch.randn(Bkv, Nk, H * D, generator=g) * 0.9
    v = torch.randn(Bkv, Nk, H * D, generator=g)
    qh, kh, vh = (_q(t, torch.bfloat16) for t in (q, k, v))
    rep = B // Bkv
    want = F.scaled_dot_product_attention(qh.view(B, Nq, H, D).transpose(1, 2),
                                          kh.view(Bkv, Nk, H, D).transpose(1, 2).repeat(rep, 1, 1, 1),
                                          vh.view(Bkv, Nk, H, D).transpose(1, 2).repeat(rep, 1, 1, 1)).transpose(1, 2).reshape(B, Nq, H * D)
    qd, kd, vd = (_dev(t, torch.bfloat16) for t in (q, k, v))
    got = eng.op_attention(qd, kd, vd, H, fp8=True).float().cpu()
    assert torch.isfinite(got).all()
    scale = float(want.abs().max())
    err = (got - want).abs()
    assert float(err.max()) <= 12e-2 * scale, (float(err.max()), scale)
    assert float(err.mean()) <= 1.5e-2 * scale, (float(err.mean()), scale)
    got16 = eng.op_attention(qd, kd, vd, H).float().cpu()
    assert float((got16 - want).abs().max()) < float(err.max())            # the bf16 kernel is the accurate one
    _attn_f64(got, q, k, v, H, torch.bfloat16, fp8=True)
    _attn_f64(got16, q, k, v, H, torch.bfloat16)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_conv3x3_vae_512px_level_on_512_row_tiles(eng, dtype):
    """The VAE's 128 -> 128 channel 3x3 conv at 512 x 512 (16-bit: 512 x 128 tiles, 8 waves as 8 x 1; bias goes straight into the
    accumulators there), plain and with a residual; checked on the image borders, the tile seams and the second image."""
    B, H, W, Cin, Cout = 2, 512, 512, 128, 128
    g = torch.Generator().manual_seed(12)
    x = torch.randn(B, H, W, Cin, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin)
    b = torch.randn(Cout, generator=g)
    r = torch.randn(B, H, W, Cout, generator=g)
    xd, rd = _dev(x, dtype), _dev(r, dtype)
    plain = eng.op_conv3x3(xd, _dev(w), _dev(b)).float().cpu()
    res = eng.op_conv3x3(xd, _dev(w), _dev(b), rd).float().cpu()
    assert torch.isfinite(plain).all() and torch.isfinite(res).all()
    rows = [0, 1, 2, 255, 256, 510, 511]                     # image rows (a 512-row tile = one image row)
    want = F.conv2d(_q(x, dtype).permute(0, 3, 1, 2), _q(w, dtype), b, padding=1).permute(0, 2, 3, 1)
    _close(plain[:, rows], want[:, rows], dtype)
    _close(res[:, rows], (want + _q(r, dtype))[:, rows], dtype)
    # the same bits whatever the batch: one image alone takes the same tiles
    one = eng.op_conv3x3(xd[1:].contiguous(), _dev(w), _dev(b), rd[1:].contiguous()).float().cpu()
    assert torch.equal(one[0], res[1])


@pytest.mark.parametrize("dtype", DTYPES)
def test_conv3x3_vae_width_many_tiles(eng, dtype):
    """The VAE's 128 -> 128 channel 3x3 conv on a large map (bf16: 256x128 tiles, 320 of them)."""
    B, H, W, Cin, Cout = 5, 128, 128, 128, 128
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B, H, W, Cin, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin)
    b = torch.randn(Cout, generator=g)
    r = torch.randn(B, H, W, Cout, generator=g)
    got = eng.op_conv3x3(_dev(x, dtype), _dev(w), _dev(b), _dev(r, dtype)).float().cpu()
    sel = [0, 4]
    want = F.conv2d(_q(x[sel], dtype).permute(0, 3, 1, 2), _q(w, dtype), b, padding=1).permute(0, 2, 3, 1) + _q(r[sel], dtype)
    _close(got[sel], want, dtype)
    assert torch.isfinite(got).all()
    _f64(got[sel], x[sel], w, dtype, conv={}, bias=b, residual=r[sel].to(dtype))


def test_linear_randomized_shapes(eng):
    """Seeded sweep over ragged M, every supported N/K granularity, bias / residual on and off, both dtypes: the
    tile / epilogue-kind / persistence choice is data-dependent, so walk many combinations."""
    rng = np.random.default_rng(7)
    for case in range(40):
        dtype = DTYPES[case % 2]
        M = int(rng.choice([1, 31, 128, 257, 1000, 4097, 20000]))
        N = int(rng.choice([64, 128, 160, 192, 256, 320, 384, 640, 1152]))
        K = int(rng.choice([64, 128, 320, 576, 1280]))
        use_bias, use_res = bool(rng.integers(2)), bool(rng.integers(2))
        g = torch.Generator().manual_seed(case)
        x = torch.randn(M, K, generator=g)
        w = torch.randn(N, K, generator=g) / math.sqrt(K)
        b = torch.randn(N, generator=g) if use_bias else None
        r = torch.randn(M, N, generator=g) if use_res else None
        want = F.linear(_q(x, dtype), _q(w, dtype), b) + (_q(r, dtype) if use_res else 0)
        got = eng.op_linear(_dev(x, dtype), _dev(w), _dev(b) if use_bias else None, _dev(r, dtype) if use_res else None)
        try:
            _close(got, want, dtype)
            _f64(got, x, w, dtype, bias=b, residual=r.to(dtype) if use_res else None)
        except AssertionError as e:
            raise AssertionError(f"case {case}: M={M} N={N} K={K} bias={use_bias} res={use_res} {dtype}: {e}")


def test_conv3x3_randomized_shapes(eng):
    """Seeded sweep over odd map sizes, channel counts, stride 2 and the folded 2x upsample, both dtypes."""
    rng = np.random.default_rng(11)
    for case in range(24):
        dtype = DTYPES[case % 2]
        B = int(rng.choice([1, 2, 5]))
        H, W = int(rng.choice([3, 8, 13, 32, 40])), int(rng.choice([4, 8, 17, 32]))
        Cin, Cout = int(rng.choice([64, 128, 320, 640])), int(rng.choice([64, 128, 160, 320]))
        mode = int(rng.integers(3))                       # 0 plain, 1 stride 2, 2 upsample
        if mode == 1 and (H % 2 or W % 2):
            H, W = H + H % 2, W + W % 2
        stride, ups = (2, False) if mode == 1 else ((1, True) if mode == 2 else (1, False))
        g = torch.Generator().manual_seed(100 + case)
        x = torch.randn(B, Cin, H, W, generator=g)
        w = torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin)
        b = torch.randn(Cout, generator=g)
        xin = _q(x, dtype)
        if ups:
            xin = F.interpolate(xin, scale_factor=2.0, mode="nearest")
        want = F.conv2d(xin, _q(w, dtype), b, stride=stride, padding=1)
        r = torch.randn(want.shape, generator=g)
        got = eng.op_conv3x3(_dev(x.permute(0, 2, 3, 1), dtype), _dev(w), _dev(b), _dev(r.permute(0, 2, 3, 1), dtype), stride, ups)
        try:
            _close(got.float().cpu().permute(0, 3, 1, 2), want + _q(r, dtype), dtype)
            _f64(got, x.permute(0, 2, 3, 1).contiguous(), w, dtype, conv=dict(stride=stride, ups=int(ups)), bias=b,
                 residual=r.permute(0, 2, 3, 1).to(dtype))
        except AssertionError as e:
            raise AssertionError(f"case {case}: B={B} H={H} W={W} Cin={Cin} Cout={Cout} stride={stride} ups={ups} {dtype}: {e}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D,scale", [(40, 3.0), (160, 2.0), (64, 3.0), (72, 3.0), (80, 3.0)])
def test_attention_peaked_logits(eng, dtype, D, scale):
    """Near one-hot softmax rows (logit standard deviation 9 = 13 in log2 units, spreads of +-50): the running-max
    re-base path runs on many key tiles and exp2 underflows for most keys -- results must stay finite and match torch.
    (Q is pre-scaled by log2(e)/sqrt(D) in the compute dtype, one extra rounding of the logits: 2^-9 relative in bf16, so
    at logit magnitudes in the hundreds the bf16 kernel's near-tie rows drift by several percent -- outside what the
    U-Net produces and outside this test.)"""
    B, H, Nq, Nk = 2, 2, 192, 333
    g = torch.Generator().manual_seed(D)
    q = torch.randn(B, Nq, H * D, generator=g) * scale
    k = torch.randn(B, Nk, H * D, generator=g) * scale
    v = torch.randn(B, Nk, H * D, generator=g)
    qh, kh, vh = (_q(t, dtype) for t in (q, k, v))
    want = F.scaled_dot_product_attention(qh.view(B, Nq, H, D).transpose(1, 2), kh.view(B, Nk, H, D).transpose(1, 2),
                                          vh.view(B, Nk, H, D).transpose(1, 2)).transpose(1, 2).reshape(B, Nq, H * D)
    got = eng.op_attention(_dev(q, dtype), _dev(k, dtype), _dev(v, dtype), H)
    assert torch.isfinite(got.float()).all()
    _close(got, want, dtype)
    _attn_f64(got, q, k, v, H, dtype)


@pytest.mark.parametrize("M,dtype", _h16_cases([128, 96, 4096 + 32, 40000]))
def test_ff_fused_320(eng, M, dtype):
    """LayerNorm -> GEGLU projection -> ff.net.2 -> + residual as ONE launch (row-resident kernel, bf16 and its fp16 twin, C = 320)
    against the fp32 CPU chain (hacked_modules.py:118-132), the float64 chain and the three-launch HIP chain it replaces."""
    C = 320
    g = torch.Generator().manual_seed(M)
    x = torch.randn(M, C, generator=g) * 1.5 + 0.3
    lg, lb = torch.randn(C, generator=g) * 0.2 + 1.0, torch.randn(C, generator=g) * 0.1
    w1 = torch.randn(8 * C, C, generator=g) / math.sqrt(C)
    b1 = torch.randn(8 * C, generator=g) * 0.5
    w2 = torch.randn(C, 4 * C, generator=g) / math.sqrt(4 * C)
    b2 = torch.randn(C, generator=g) * 0.5
    xq = _q(x, dtype)
    n = _q(F.layer_norm(xq, (C,), lg, lb, 1e-5), dtype)
    hh, gg = F.linear(n, _q(w1, dtype), b1).chunk(2, dim=-1)
    hid = _q(hh * F.gelu(gg), dtype)
    want = xq + F.linear(hid, _q(w2, dtype), b2)
    xd = _dev(x, dtype)
    got = eng.op_ff_fused(xd, _dev(lg), _dev(lb), _dev(w1), _dev(b1), _dev(w2), _dev(b2))
    _close(got, want, dtype)
    _rowres_f64(eng, got, xd, lg, lb, dtype, ff=(w1, b1, w2, b2))
    # the unfused HIP chain on the same inputs: same roundings at the same places, so the two agree much tighter than the gate
    n_h = eng.op_layernorm(xd, _dev(lg), _dev(lb), 1e-5)
    hid_h = eng.op_linear(n_h, _dev(w1), _dev(b1), None, geglu=True)
    ref_h = eng.op_linear(hid_h, _dev(w2), _dev(b2), xd)
    d = (got.float() - ref_h.float()).abs().max().item()
    assert d <= float(want.abs().max()) / 64, d       # two bf16 ulps of the largest output
    # in place (out aliases x), as the U-Net executor calls it; and bit-reproducible
    L = eng._lib.lib()
    x2 = xd.clone()
    ws = [_dev(t) for t in (lg, lb, w1, b1, w2, b2)]
    ptrs = [x2.data_ptr()] + [w.data_ptr() for w in ws] + [x2.data_ptr()]
    if dtype == torch.bfloat16:        # the entry point without a dtype argument is bf16's
        eng._lib.check(L.dsim_op_ff_fused(*ptrs, M, C, 1e-5, None), "ff in place")
    else:
        eng._lib.check(L.dsim_op_ff_fused_dt(*ptrs, M, C, 1e-5, eng._TORCH2DSIM[dtype], None), "ff in place")
    assert torch.equal(x2, got)


@pytest.mark.parametrize("M,N,ln,dtype", _h16_cases([(128, 960, True), (96, 320, True), (4096 + 32, 960, True), (40000, 320, True),
                                                      (1000, 640, False), (33, 64, True)]))
def test_ln_linear_320(eng, M, N, ln, dtype):
    """LayerNorm -> bias-free Linear as ONE launch (row-resident kernel, bf16 and its fp16 twin, C = 320): norm1 -> to_q|to_k|to_v
    (N = 960) and norm2 -> attn2.to_q (N = 320) of hacked_modules.py:88-116, against the fp32 CPU chain, against float64 stage by
    stage, and against the two-launch HIP chain it replaces (same rounding points: the normalised row is rounded to the 16-bit type
    before the GEMM in both)."""
    C = 320
    g = torch.Generator().manual_seed(M + N)
    x = torch.randn(M, C, generator=g) * 1.5 + 0.3
    lg, lb = torch.randn(C, generator=g) * 0.2 + 1.0, torch.randn(C, generator=g) * 0.1
    w = torch.randn(N, C, generator=g) / math.sqrt(C)
    xq = _q(x, dtype)
    n = _q(F.layer_norm(xq, (C,), lg, lb, 1e-5), dtype) if ln else xq
    want = F.linear(n, _q(w, dtype))
    xd = _dev(x, dtype)
    got = eng.op_ln_linear(xd, _dev(lg) if ln else None, _dev(lb) if ln else None, _dev(w))
    assert got.shape == (M, N)
    _close(got, want, dtype)
    _rowres_f64(eng, got, xd, lg if ln else None, lb if ln else None, dtype, w=w)
    n_h = eng.op_layernorm(xd, _dev(lg), _dev(lb), 1e-5) if ln else xd
    ref_h = eng.op_linear(n_h, _dev(w), None, None)
    d = (got.float() - ref_h.float()).abs().max().item()
    assert d <= float(want.abs().max()) / 64, d
    if not ln:
        assert torch.equal(got, ref_h)         # same MFMA k order, no other rounding point: bit for bit
    assert torch.equal(got, eng.op_ln_linear(xd, _dev(lg) if ln else None, _dev(lb) if ln else None, _dev(w)))
    for bad in ((C, 100), (C, 1024), (256, 320)):
        with pytest.raises(eng._lib.DsimError):
            eng.op_ln_linear(torch.zeros(8, bad[0], dtype=dtype, device="cuda"), None, None, torch.zeros(bad[1], bad[0], device="cuda"))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("Nq,Nk", [(300, 2048), (256, 4096), (300, 4096)])
def test_attention_pipelined_kernel_takes_the_exact_fallback(eng, Nq, Nk, dtype):
    """attn_long_kernel itself (bf16, d = 40, Nk >= 2048 and Nk % 64 == 0: SD1.5's 4096-key self-attention, the headline path)
    through its exact-softmax fallback: the forced cases of test_attention_long_keys_fixed_reference_softmax use Nk = 2048 + 77,
    which routes to attn_kernel / attend_checked.  Here the spike sits at a key far down a sequence the pipelined kernel owns, so
    its __syncthreads_or(bad) and the two exact re-runs over the 3-deep ring execute; ragged Nq exercises the partial last
    query block through the same path.  The spiked workgroup and an un-spiked one (other head, other query block) are checked.
    In fp16 the "late spike" (P = 2^40 relative to tile 0) already exceeds the type's range, so it takes the fallback too."""
    B, H, D = 1, 2, 40
    g = torch.Generator().manual_seed(Nq + Nk)
    q = torch.randn(B, Nq, H * D, generator=g)
    k = torch.randn(B, Nk, H * D, generator=g)
    v = torch.randn(B, Nk, H * D, generator=g)
    key = Nk - 500
    rows = (7, Nq - 3)                      # one row in the first query block, one in the (ragged) last
    for case, boost in (("plain", 0.0), ("late spike", 28.0), ("overflow", 210.0)):
        kk = k.clone()
        qq = q.clone()
        if boost:
            # both spiked rows share one direction in head 0, so ONE key gives both the logit `boost` (natural units)
            qq[0, rows[1], :D] = qq[0, rows[0], :D]
            q7 = qq[0, rows[0], :D]
            kk[0, key, :D] = boost * q7 / (q7.norm() ** 2) * math.sqrt(D)
        qh, kh, vh = (_q(t, dtype) for t in (qq, kk, v))
        want = F.scaled_dot_product_attention(qh.double().view(B, Nq, H, D).transpose(1, 2), kh.double().view(B, Nk, H, D).transpose(1, 2),
                                              vh.double().view(B, Nk, H, D).transpose(1, 2)).transpose(1, 2).reshape(B, Nq, H * D).float()
        got = eng.op_attention(_dev(qq, dtype), _dev(kk, dtype), _dev(v, dtype), H)
        assert got.shape == (B, Nq, H * D)
        assert torch.isfinite(got.float()).all(), case
        _attn_f64(got, qq, kk, v, H, dtype)
        if case == "overflow":
            assert (got.float().cpu() - want).abs().max().item() <= 5e-2 * float(want.abs().max())
        else:
            _close(got, want, dtype)
        # head 1 never sees the spike: the same numbers whichever path its neighbour took
        _close(got[..., D:], want[..., D:], dtype)
        if boost:
            for r in rows:                  # the spiked rows are one-hot on `key`
                assert (got[0, r, :D].float().cpu() - vh[0, key, :D]).abs().max().item() < 2e-2, (case, r)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("Nk", [2048 + 77, 1024])
@pytest.mark.parametrize("D", [40, 64, 80])
def test_attention_long_keys_fixed_reference_softmax(eng, D, Nk, dtype):
    """Key sequences >= 1024 take the fixed-reference softmax (the maximum is fixed after key tile 0, later tiles never look
    at their scores; attn_core.h attend<FAST>).  (1) ordinary data; (2) the rare branch, FORCED (cdna_hip_programming.md rule
    26): one key far down the sequence scores ~+40 (log2 units) above everything in tile 0 for some rows -> P up to 2^40,
    still exact after normalisation; (3) a key ~+300 above -> exp2 overflows in the fast form, the end-of-block check must
    send the workgroup through the exact running-maximum form.  All against float64 SDPA over the whole tensor."""
    B, H, Nq = 1, 2, 256
    key = 1500 if Nk > 1500 else 900
    g = torch.Generator().manual_seed(D)
    q = torch.randn(B, Nq, H * D, generator=g)
    k = torch.randn(B, Nk, H * D, generator=g)
    v = torch.randn(B, Nk, H * D, generator=g)
    for case, boost in (("plain", 0.0), ("late spike", 28.0), ("overflow", 210.0)):
        kk = k.clone()
        if boost:       # key `key` of head 0 aligned with query row 7 of head 0: its logit is `boost` (natural units) exactly
            q7 = q[0, 7, :D]
            kk[0, key, :D] = boost * q7 / (q7.norm() ** 2) * math.sqrt(D)
        qh, kh, vh = (_q(t, dtype) for t in (q, kk, v))
        want = F.scaled_dot_product_attention(qh.double().view(B, Nq, H, D).transpose(1, 2), kh.double().view(B, Nk, H, D).transpose(1, 2),
                                              vh.double().view(B, Nk, H, D).transpose(1, 2)).transpose(1, 2).reshape(B, Nq, H * D).float()
        got = eng.op_attention(_dev(q, dtype), _dev(kk, dtype), _dev(v, dtype), H)
        assert torch.isfinite(got.float()).all(), case
        _attn_f64(got, q, kk, v, H, dtype)
        if case == "overflow":
            # logits in the hundreds: the documented drift of near-tie rows under the bf16 pre-scaled Q (test_attention_peaked_logits)
            # applies to the exact form too; here the point is that the fallback ran: finite, and within 5 % of the range
            assert (got.float().cpu() - want).abs().max().item() <= 5e-2 * float(want.abs().max())
        else:
            _close(got, want, dtype)
        if boost:                   # the spiked row is one-hot on `key`
            assert (got[0, 7, :D].float().cpu() - vh[0, key, :D]).abs().max().item() < 2e-2, case
