"""A float64 restatement of the kernels in front of the models -- csrc/pack.hip (noising + conv_in in its three kernels, the
sinusoidal embeddings, the time-embedding GEMV, the four weight packs, dup_batch, resize_nearest, gather_ctx), the patch embedding of
csrc/dit.hip and the quant_conv fold and output transpose of csrc/vae.hip -- and the per-element error bound of each arithmetic one,
shared by tests/test_front64_host.py and tests/test_gpu_front64.py.  Not a conftest: import it like tests/_gemm64.py.

The semantics are the models'.
  * conv_in: x_t = sa lat + sb noise (DDPM add_noise; lat alone where there is no noise), then nn.Conv2d(Cin, Cout, 3, padding=1), the
    result token-major and each image written `dup` times in a row (the classifier-free-guidance copies [img * dup + d]).
  * patch embedding: the same x_t, DiT's PatchEmbed (a p x p conv of stride p, flattened row-major over the token grid) + pos_embed,
    both CFG halves.
  * GroupNorm partials of the row kernel: f32 (sum, sum of squares) of the STORED values per (64-pixel chunk, 4-channel quad), the
    layout of a conv epilogue's gn_part; their bound is tests/test_gpu_gemm64.py's _check_gn (256 terms, worst case), reused there.
  * sinusoidal embeddings: diffusers Timesteps(dim, flip_sin_to_cos=True, downscale_freq_shift=0): [cos | sin](t f_i), f_i =
    exp(-ln(10000) i / half), half = dim / 2.
  * GEMV: y = W act(x) + bias, act = SiLU on the INPUT when act == 1 (TimestepEmbedding's linear_2(silu(linear_1(.))), DiT's adaLN).
  * fold_quant: quant_conv (1x1) after conv_out, both linear: W' = Wq Wco, b' = Wq bco + bq.
Operands are taken as the kernel receives them: f32 inputs, the f32 values of sa and sb, weights in the dtype they are stored in.
Everything else is float64.

THE BOUNDS.  U32 = 2^-24, gam(n) = n U32 / (1 - n U32) (Higham, Accuracy and Stability of Numerical Algorithms, Lemma 3.1: n
roundings compound to at most gam(n) relative).  K <= 64 everywhere here, so these are the deterministic worst-case bounds, not the
probabilistic ones of tests/_gemm64.py.  Every arithmetic output then takes one rounding to the output dtype, composed as
tests/_gemm64.py composes it: u_out |ref| + (1 + u_out) E (+ 2^-25 in fp16: half the spacing of its subnormals).

conv_in / patch embedding, E =
  * noising.  `sa * lat[o] + sb * noise[o]`: two products and a sum, or a product and an fma as the compiler contracts it; either way
    each product carries at most one rounding and the sum one: |dv| <= 2 U32 (|sa lat| + |sb noise|).  It reaches the output through
    the weights: sum_k dv_k |w_k|.  Nothing where noise is null (the value is loaded).
  * the chain.  `acc = bias; acc = fmaf(patch, w, acc)` K times in ascending k (K = 9 Cin or Cin p^2): K roundings of partial sums
    that are each at most s = sum|a||w| + |bias| in magnitude: gam(K + 1) s (the issue's count, K + 1; the chain itself has K).
    A tap outside the image multiplies an exact zero.
  * the position add of the patch embedding, `acc + pos`: one more rounding of a value of at most s + |pos|: gam(K + 2) (s + |pos|)
    covers chain and add.
sinusoidal embeddings.  `f = expf(-logf(10000.0f) * (float)i / (float)half); e = (float)t * f; cosf(e), sinf(e)`.
  The HIP documentation's table of device math accuracy (docs/reference/math_api) does not ship with the ROCm packages (their
  share/doc/hip holds the Doxygen runtime API only), so the figures are ASSUMED: the device functions are OCML's, which are built to
  the OpenCL full profile, and the OpenCL 3.0 C specification, section 7.4 (relative error as ULP), gives exp <= 3 ulp, log <= 3 ulp,
  sin / cos <= 4 ulp.  One ulp is at most 2 U32 relative.
  * the exponent a = -ln(10000) i / half: logf 3 ulp (6 U32) unless folded at compile time, the product and the division one
    rounding each: |da| <= 8 U32 |a|.  exp(a + da) = f exp(da): relative 8 U32 |a| = 8 U32 |ln f|.
  * expf: 3 ulp, 6 U32 relative.  The product with t (exact as an f32 below 2^24; a value of sincos_values is an f32 already): U32.
    Together the argument is off by |de| <= e (8 |ln f| + 7) U32 (1 + 1e-5: the second-order remainder of exp(da), da < 5e-6):
    proportional to t f |ln f|, largest at f = 1 / e.
  * cosf / sinf: slope at most 1, so |de| goes through unamplified; their own 4 ulp, 8 U32 (|ref| + |de|), which includes the rounding
    of the result to f32 (there is no further store rounding: the output is f32).
GEMV.  One wave per row: lane l sums k = l, l + 64, ... by fmaf from 0 (n_l = ceil(K / 64) roundings), six xor-shuffle adds, the bias
  add: no operand passes through more than n_l + 7 roundings: gam(n_l + 7) (sum|w||act(x)| + |bias|).  SiLU as `x / (1.0f + expf(-x))`:
  expf 3 ulp on E = exp(-x), which moves 1 + E by 6 U32 E / (1 + E) <= 6 U32 relative, the addition and the (correctly rounded: no
  fast-math flag in diffsim_amd/build.py) division one rounding each: 8 U32 |silu(x)|, carried through |w|; where E overflows (x <
  -88.7) the quotient is -0 for a true value below 89 x 2^-128: 2^-120 |w| covers it.
fold_quant.  `acc = fmaf(wq, wco, acc)` from 0 over Cm terms: gam(Cm) sum|wq||wco|, then the rounding to the compute dtype; the bias
  from bq: gam(Cm) (sum|wq||bco| + |bq|), f32 out.
The packs, to_nchw_f32, dup_batch, gather_ctx and resize_nearest are index permutations with at most one round-to-nearest-even
conversion (torch's .to()): they have no bound and are compared with torch.equal.

emulate_*() replay each arithmetic kernel in float32 on the CPU in the kernel's operation order as far as torch allows (an fma is
formed in float64 and rounded once more, as tests/_norm64.py's _fma32).  They exist so that tests/test_front64_host.py can hold the
REFERENCE SIDE ALONE to the bounds on the GPU test's own case list before any GPU time is spent."""
import math

import numpy as np
import torch
import torch.nn.functional as F

U = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
U32 = 2.0 ** -24
F16_FLOOR = 2.0 ** -25          # half the spacing of fp16's subnormals
ULP_EXP, ULP_LOG, ULP_SINCOS = 3, 3, 4      # OpenCL 3.0 C section 7.4 (assumed for the OCML device functions; see the docstring)
SILU_TINY = 2.0 ** -120
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


def gam(n):
    return n * U32 / (1 - n * U32)


def out_bound(ref, E, dtype):
    u = U[dtype]
    b = u * ref.abs() + (1 + u) * E
    return b + F16_FLOOR if dtype == torch.float16 else b


def check(got, ref, bound, what=""):
    """Returns the largest err / bound; raises with the worst element on any violation (tests/_norm64.py check())."""
    from tests import _norm64
    return _norm64.check(got, ref, bound, what)


# ---- conv_in and the patch embedding ---------------------------------------------------------------------------------------------
def noised(lat, noise, sa, sb):
    """(x_t, |dx_t| bound) float64: sa, sb as their f32 values"""
    if noise is None:
        return lat.double(), torch.zeros_like(lat, dtype=torch.float64)
    sa, sb = float(np.float32(sa)), float(np.float32(sb))
    a, b = sa * lat.double(), sb * noise.double()
    return a + b, 2 * U32 * (a.abs() + b.abs())


def conv_in_ref_and_bound(lat, noise, sa, sb, w, bias, dtype, dup=1, rows=None):
    """lat / noise f32 [n][Cin][S][S], w f32 [Cout][Cin][3][3], bias f32 [Cout] -> (ref, bound) float64 [n * dup][S * S][Cout], the
    copies of image i at [i * dup + d].  rows: a sorted int64 tensor of image rows y to reference (the output is then
    [n * dup][len(rows) * S][Cout]); None: all."""
    x, dx = noised(lat, noise, sa, sb)
    n, Cin, S, _ = x.shape
    wd, bd = w.to(x.device).double(), bias.to(x.device).double()
    Cout = wd.shape[0]
    if rows is not None:                                            # the three input rows of each output row, gathered (zero outside)
        rows = rows.to(x.device)
        yy = rows.view(-1, 1) + torch.arange(-1, 2, device=x.device).view(1, 3)
        ok = ((yy >= 0) & (yy < S)).double().view(1, 1, -1, 3, 1)

        def conv(t, ww):
            win = t[:, :, yy.clamp(0, S - 1)] * ok                  # [n][Cin][R][3][S]
            return torch.cat([F.conv2d(win[:, :, r], ww, padding=(0, 1)) for r in range(len(rows))], 2)
    else:
        conv = lambda t, ww: F.conv2d(t, ww, padding=1)
    y = conv(x, wd) + bd.view(1, -1, 1, 1)
    s = conv(x.abs(), wd.abs()) + bd.abs().view(1, -1, 1, 1)
    E = gam(9 * Cin + 1) * s + conv(dx, wd.abs())
    tok = lambda t: t.permute(0, 2, 3, 1).reshape(n, -1, Cout).repeat_interleave(dup, 0)
    ref = tok(y)
    return ref, out_bound(ref, tok(E), dtype)


def patch_ref_and_bound(lat, noise, sa, sb, w, bias, pos, p, dtype):
    """DiT's patch embedding: w f32 [D][Cin][p][p], pos f32 [T][D] -> (ref, bound) float64 [2 n][T][D]"""
    x, dx = noised(lat, noise, sa, sb)
    n, Cin = x.shape[:2]
    wd, bd, pd = w.to(x.device).double(), bias.to(x.device).double(), pos.to(x.device).double()
    D = wd.shape[0]
    y = F.conv2d(x, wd, stride=p) + bd.view(1, -1, 1, 1)
    s = F.conv2d(x.abs(), wd.abs(), stride=p) + bd.abs().view(1, -1, 1, 1)
    tok = lambda t: t.permute(0, 2, 3, 1).reshape(n, -1, D)
    ref = tok(y) + pd.view(1, -1, D)
    E = gam(Cin * p * p + 2) * (tok(s) + pd.abs().view(1, -1, D)) + tok(F.conv2d(dx, wd.abs(), stride=p))
    ref, E = ref.repeat_interleave(2, 0), E.repeat_interleave(2, 0)
    return ref, out_bound(ref, E, dtype)


def _fma32(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def _noised32(lat, noise, sa, sb):
    if noise is None:
        return lat.float()
    return torch.tensor(sa, dtype=torch.float32) * lat + torch.tensor(sb, dtype=torch.float32) * noise


def emulate_conv_in(lat, noise, sa, sb, w, bias, dtype, dup=1):
    """the direct conv replayed in float32: bias first, then the taps in ascending k = tap * Cin + ci"""
    x = F.pad(_noised32(lat, noise, sa, sb), (1, 1, 1, 1))
    n, Cin, S = lat.shape[:3]
    Cout = w.shape[0]
    acc = bias.float().view(1, 1, 1, Cout).expand(n, S, S, Cout).contiguous()
    for tap in range(9):
        for ci in range(Cin):
            a = x[:, ci, tap // 3:tap // 3 + S, tap % 3:tap % 3 + S].unsqueeze(-1)
            acc = _fma32(a, w[:, ci, tap // 3, tap % 3].float().view(1, 1, 1, Cout), acc)
    return acc.reshape(n, S * S, Cout).to(dtype).repeat_interleave(dup, 0)


def emulate_patch_embed(lat, noise, sa, sb, w, bias, pos, p, dtype):
    x = _noised32(lat, noise, sa, sb)
    n, Cin, S = lat.shape[:3]
    g, D = S // p, w.shape[0]
    acc = bias.float().view(1, 1, 1, D).expand(n, g, g, D).contiguous()
    for c in range(Cin):
        for py in range(p):
            for px in range(p):
                a = x[:, c, py::p, px::p].unsqueeze(-1)
                acc = _fma32(a, w[:, c, py, px].float().view(1, 1, 1, D), acc)
    out = (acc.reshape(n, g * g, D) + pos.float().view(1, g * g, D)).to(dtype)
    return out.repeat_interleave(2, 0)


def gn_partials64(stored):
    """float64 (sum, sum of squares) of the stored values [n][HW][C] per (64-pixel chunk, 4-channel quad): [n][HW / 64][C / 4][2]"""
    n, HW, Cc = stored.shape
    q = stored.double().view(n, HW // 64, 64, Cc // 4, 4)
    return torch.stack([q.sum((2, 4)), (q * q).sum((2, 4))], -1)


# ---- sinusoidal embeddings -------------------------------------------------------------------------------------------------------
def sincos_ref_and_bound(dim, vals):
    """vals: the t values as the kernel holds them (f32-exact floats) -> (ref, bound) float64 [len(vals)][dim] = [cos | sin]"""
    half = dim // 2
    t = torch.as_tensor(vals, dtype=torch.float32).cpu().double().view(-1, 1)
    a = -math.log(10000.0) * torch.arange(half, dtype=torch.float64) / half
    e = t * torch.exp(a).view(1, -1)
    ref = torch.cat([torch.cos(e), torch.sin(e)], 1)
    de = e.abs() * ((2 * ULP_LOG + 2) * a.abs().view(1, -1) + 2 * ULP_EXP + 1) * U32 * (1 + 1e-5)
    de = torch.cat([de, de], 1)
    return ref, de + 2 * ULP_SINCOS * U32 * (ref.abs() + de)


def emulate_sincos(dim, vals):
    half = dim // 2
    i = torch.arange(half, dtype=torch.float32)
    f = torch.exp(-torch.log(torch.tensor(10000.0, dtype=torch.float32)) * i / torch.tensor(float(half), dtype=torch.float32))
    e = torch.as_tensor(vals, dtype=torch.float32).view(-1, 1) * f.view(1, -1)
    return torch.cat([torch.cos(e), torch.sin(e)], 1)


# ---- GEMV ------------------------------------------------------------------------------------------------------------------------
def gemv_ref_and_bound(W, bias, x, act):
    """W [N][K] / bias [N] in their stored dtypes, x f32 [K] -> (ref, bound) float64 [N]"""
    Wd, xd = W.double(), x.double()
    K = Wd.shape[1]
    ax = F.silu(xd) if act == 1 else xd
    bd = bias.double() if bias is not None else torch.zeros(Wd.shape[0], dtype=torch.float64, device=Wd.device)
    ref = Wd @ ax + bd
    s = Wd.abs() @ ax.abs() + bd.abs()
    E = gam(-(-K // 64) + 7) * s
    if act == 1:
        E = E + (2 * ULP_EXP + 2) * U32 * (Wd.abs() @ ax.abs()) + SILU_TINY * Wd.abs().sum(1)
    return ref, E                   # f32 out: the last rounding is the bias add's, counted above


def emulate_gemv(W, bias, x, act):
    """lane l's fmaf chain over k = l, l + 64, ..., the xor-shuffle tree, the bias add"""
    Wf, xf = W.float(), x.float()
    N, K = Wf.shape
    if act == 1:
        xf = xf / (1.0 + torch.exp(-xf))
    n_l = -(-K // 64)
    Wp, xp = torch.zeros(N, n_l * 64), torch.zeros(n_l * 64)
    Wp[:, :K], xp[:K] = Wf, xf
    acc = torch.zeros(N, 64)
    for j in range(n_l):
        acc = _fma32(Wp[:, 64 * j:64 * j + 64], xp[64 * j:64 * j + 64].view(1, 64), acc)
    lanes, o = torch.arange(64), 32
    while o:
        acc = acc + acc[:, lanes ^ o]
        o //= 2
    return acc[:, 0] + (bias.float() if bias is not None else 0.0)


# ---- fold_quant ------------------------------------------------------------------------------------------------------------------
def fold_ref_and_bound(wq, wco, dtype):
    """wq f32 [Cm][Cm], wco [Cm][K] in the compute dtype -> (ref, bound) float64 [Cm][K]"""
    a, b = wq.double(), wco.double()
    ref = a @ b
    return ref, out_bound(ref, gam(a.shape[1]) * (a.abs() @ b.abs()), dtype)


def fold_bias_ref_and_bound(wq, bco, bq):
    a, b, c = wq.double(), bco.double(), bq.double()
    return a @ b + c, gam(a.shape[1]) * (a.abs() @ b.abs() + c.abs())


def emulate_fold(wq, wco, dtype):
    acc = torch.zeros(wq.shape[0], wco.shape[1])
    for c in range(wq.shape[1]):
        acc = _fma32(wq[:, c].float().view(-1, 1), wco[c].float().view(1, -1), acc)
    return acc.to(dtype)


def emulate_fold_bias(wq, bco, bq):
    acc = bq.float().clone()
    for c in range(wq.shape[1]):
        acc = _fma32(wq[:, c].float(), bco[c].float(), acc)
    return acc


# ---- the exact operators ---------------------------------------------------------------------------------------------------------
def geglu_src_rows(N, rows):
    """the source row of each packed row: diffusers' [h (0..F) ; g (F..2F)] as alternating blocks of `rows` rows [h0, g0, h1, ...]"""
    n = torch.arange(N)
    blk, within = n // rows, n % rows
    j = (blk // 2) * rows + within
    return torch.where(blk % 2 == 1, N // 2 + j, j)


def pack_ref(kind, src, dst_dtype, geglu=0):
    """the packed tensor: an index permutation, then ONE round-to-nearest-even conversion (16-bit sources are exact in f32)"""
    if kind in ("linear", "vector"):
        out = src[geglu_src_rows(src.shape[0], geglu).to(src.device)] if geglu else src
    elif kind == "conv3":                                   # [Co][Ci][3][3] -> [Co][tap][Ci]
        out = src.reshape(src.shape[0], src.shape[1], 9).permute(0, 2, 1)
    else:                                                   # conv_in: -> [tap * Ci + ci][Co]
        out = src.reshape(src.shape[0], src.shape[1], 9).permute(2, 1, 0).reshape(9 * src.shape[1], src.shape[0])
    return out.float().to(dst_dtype).contiguous()


def nearest_index(n_in, n_out):
    """torch's nearest source index, restated with integers and ONE f32 scale: min(floor(dst * (float)in / out), in - 1)"""
    scale = np.float32(n_in) / np.float32(n_out)
    return torch.tensor([min(int(np.floor(np.float32(d) * scale)), n_in - 1) for d in range(n_out)], dtype=torch.int64)


def resize_ref(x, Hout, Wout):
    """x [B][Hin][Win][C] -> [B][Hout][Wout][C]"""
    iy, ix = nearest_index(x.shape[1], Hout).to(x.device), nearest_index(x.shape[2], Wout).to(x.device)
    return x[:, iy][:, :, ix].contiguous()


def resize_ref_torch(x, Hout, Wout):
    """the same through F.interpolate(mode="nearest") on the NCHW view (float32 carries any 16-bit value exactly)"""
    y = F.interpolate(x.float().permute(0, 3, 1, 2), size=(Hout, Wout), mode="nearest")
    return y.permute(0, 2, 3, 1).to(x.dtype).contiguous()


def dup_ref(x):
    return x.repeat_interleave(2, 0)


def gather_ref(ctx, index, dtype):
    """ctx f32 [n_ctx][2][...], index int [n] -> [2 n][...]: row 2 i + cfg = ctx[clamp(index[i], 0, n_ctx - 1)][cfg]"""
    c = index.long().clamp(0, ctx.shape[0] - 1)
    return ctx[c].reshape((2 * index.numel(),) + tuple(ctx.shape[2:])).to(dtype)


def nchw_ref(x):
    return x.float().permute(0, 2, 1).contiguous()


# ---- the case lists, shared by the host and the GPU tests -------------------------------------------------------------------------
# conv_in: (Cin, S, Cout) -> the kernel the executors' choice must report
CONV_IN_CASES = {
    (4, 8, 320): "eight", (4, 7, 320): "eight", (4, 13, 32): "eight", (3, 16, 128): "eight", (4, 5, 2048): "eight", (4, 5, 1288): "eight",
    (4, 9, 8): "generic", (4, 9, 100): "generic", (4, 9, 132): "generic", (4, 9, 300): "generic",
}
SINCOS_DIMS = (32, 256, 320, 1280)
SINCOS_T = (0, 1, 261, 600, 667, 999, 1000)
SINCOS_VALUES = {"sdxl_1024": (1024.0, 1024.0, 0.0, 0.0, 1024.0, 1024.0), "sdxl_512": (512.0, 512.0, 0.0, 0.0, 512.0, 512.0),
                 "fractional": (0.5, 3.25, 17.125, 333.3330078125, 999.5, 1e-3)}
# (N, K): every N at two values of K, every K at two values of N
GEMV_SHAPES = ((1, 1), (1, 64), (3, 63), (3, 1280), (4, 1), (4, 65), (5, 63), (5, 320), (1280, 320), (1280, 2816), (6912, 64), (6912, 1280),
               (4, 2816), (5, 65))
PATCH_CASES = ((4, 32, 2, 1152), (4, 10, 2, 384), (4, 6, 2, 100), (4, 8, 4, 256))          # (Cin, S, p, D)
FOLD_CASES = ((8, 4608), (8, 300))


def _g(seed):
    return torch.Generator().manual_seed(seed)


def conv_in_inputs(Cin, S, Cout, n_img, seed=0):
    g = _g(1000 * Cin + 10 * S + Cout + n_img + seed)
    lat, noise = torch.randn(n_img, Cin, S, S, generator=g), torch.randn(n_img, Cin, S, S, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin)
    bias = 0.1 * torch.randn(Cout, generator=g)
    return lat, noise, 0.8365, 0.5479, w, bias           # sa, sb: sqrt(abar), sqrt(1 - abar) near t = 400


def patch_inputs(Cin, S, p, D, n_img):
    g = _g(7 * S + D + n_img)
    T = (S // p) ** 2
    lat, noise = torch.randn(n_img, Cin, S, S, generator=g), torch.randn(n_img, Cin, S, S, generator=g)
    w = torch.randn(D, Cin, p, p, generator=g) / math.sqrt(Cin * p * p)
    return lat, noise, 0.8365, 0.5479, w, 0.1 * torch.randn(D, generator=g), torch.randn(T, D, generator=g)


def gemv_inputs(N, K, wdt, bdt, seed=0):
    """x carries large magnitudes (SiLU's tails: +-30, +-90, +-100 where K allows) among randn"""
    g = _g(31 * N + K + seed)
    W = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(wdt)
    bias = None if bdt is None else torch.randn(N, generator=g).to(bdt)
    x = 2.0 * torch.randn(K, generator=g)
    tails = torch.tensor([30.0, -30.0, 90.0, -90.0, 100.0, -100.0, -88.0, 1e-4])
    m = min(K, len(tails))
    x[torch.randperm(K, generator=g)[:m]] = tails[:m]
    return W, bias, x


def fold_inputs(Cm, K, dtype):
    g = _g(Cm + K)
    return (torch.randn(Cm, Cm, generator=g) / math.sqrt(Cm), (torch.randn(Cm, K, generator=g) * 0.05).to(dtype),
            0.1 * torch.randn(Cm, generator=g), 0.1 * torch.randn(Cm, generator=g))


def pack_source(shape, sdt, seed=0):
    """values over several binades, with round-to-nearest-even ties of both 16-bit types planted where the source type holds them"""
    g = _g(sum(shape) + seed)
    x = torch.randn(shape, generator=g) * torch.exp2(torch.randint(-6, 7, shape, generator=g).float())
    ties = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 65504.0, 6.1e-5, 0.0])
    flat = x.view(-1)
    m = min(flat.numel(), len(ties))
    flat[torch.randperm(flat.numel(), generator=g)[:m]] = ties[:m]
    return x.to(sdt)
