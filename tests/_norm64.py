"""A float64 restatement of the normalization kernels (csrc/norm.hip: GroupNorm(+SiLU) in its one-pass, two-pass and precomputed-
statistics forms, the affine LayerNorm in its lanes-per-row and wave-per-row forms, DiT's modulated LayerNorm; and the LayerNorm
stages written again inside csrc/rowres.hip) and their per-element error bound, shared by the norm tests.  Not a conftest: import it
like tests/_gemm64.py.

The semantics are the models': GroupNorm is nn.GroupNorm over the channel concatenation cat([x0, x1]) of a token-major [B][HW][C]
map (biased variance over the HW x C / groups elements of a group, eps inside the square root), followed by F.silu where the resnets
fuse it; LayerNorm is nn.LayerNorm over the last dimension; the modulated form is DiT's norm(x) * (1 + scale) + shift with scale /
shift of the row's CFG half, half = (row // rows_per_batch) & 1 (oracle/cpu_ref.py _DiTBlock).  Operands are taken as the kernel sees
them: x in the compute dtype, gamma / beta / scale / shift f32, all as float64; eps is the model's Python float (the kernel receives it
as an f32: a term of the bound).  Everything else is float64 on the device the tensors live on.

THE BOUND.  Per element, with y the value before SiLU (or the output where there is none):

    |got - ref| <= u_out |ref| + (1 + u_out) E   (+ 2^-25, fp16's subnormal spacing / 2)

u_out is the store's rounding (2^-24 f32, 2^-8 bf16, 2^-11 fp16); the kernel rounds ITS value, which is off by E.  U32 = 2^-24;
LAM = 8 is the constant of Higham and Mary's probabilistic bound (SIAM J. Sci. Comput. 41(5), 2019, Theorem 3.1: a sum of n terms in
which rounding errors are independent and mean-zero is off by at most lam sqrt(n) u sum|terms| with probability >= 1 - 2 n
exp(-lam^2 / 2)), chosen from that statement as in tests/_gemm64.py and tests/_attn64.py, not fitted to the kernels.

GroupNorm (gn_stats_kernel / gn_onepass_kernel / gn_fold_kernel, then gn_apply_kernel or the one-pass kernel's own apply), E_y =
  * statistics.  `s1[k][e] += f; s2[k][e] = fmaf(f, f, s2[k][e])`: each thread keeps f32 running sums over the rows it walks, at most
    n_p of them (n_p = ceil(slab rows / R) in gn_stats_kernel with slab rows = ceil(HW / chunks); ceil(HW / R) in gn_onepass_kernel;
    256 terms in an unknown order for one gn_part slot of a conv epilogue).  The square is exact inside the fma.  The partials go
    through LDS to an f64 fold (`a += (double)pr.x`), whose error (2^-53 per step) is invisible.  No operand passes through more than
    n_p f32 additions: |dS1| <= LAM U32 sqrt(n_p) sum|x|, |dS2| <= LAM U32 sqrt(n_p) sum x^2 over the group.  `mean = a / n;
    var = q / n - mean * mean` in f64: dmean = dS1 / n, dvar = dS2 / n + 2 |mean| dmean.  Relative to var this is
    LAM U32 sqrt(n_p) (2 + 3 mean^2 / var)-ish: THE AMPLIFICATION of E[x^2] - mean^2 is mean^2 / var, 1024 at |mean| / std = 32.
    Through rstd = (var + eps)^-1/2 the output moves by |gamma| (rstd_w dmean + |x - mean| rstd_w^3 dvar / 2), where rstd_w =
    (max(var - dvar, 0) + eps)^-1/2 is the largest rstd on the interval the variance can lie in (mean value theorem: no first-order
    approximation here, because dvar need not be small against var + eps in a nearly constant group).
  * eps.  `float eps` -> `(double)eps`: the kernel's eps is the f32 nearest the model's, off by U32 eps; rstd moves by
    U32 eps / (2 (var + eps)) relative.  First order only where the variance is tiny.
  * affine.  `s_mean[g] = (float)mean; s_rstd[g] = (float)(1.0 / sqrt(var + eps))`, `w = gamma[c] * s_rstd[g]`,
    `sh = beta[c] - s_mean[g] * w`, `fmaf(x, w, sh)`: the cast of rstd and the product make w off by 2 U32 relative, common to x w
    and mean w, so 2 U32 |x - mean| rstd |gamma|; the cast of mean, the product mean w and the subtraction are absolute:
    U32 |mean| rstd |gamma| each for the first two, U32 (|mean| rstd |gamma| + |beta|) for the third (two roundings or one, as the
    compiler contracts it: the same bound); the fma U32 |y|.  Together 2 U32 |x - mean| rstd |gamma| + 3 U32 |mean| rstd |gamma| +
    U32 |beta| + U32 |y|.  (The issue's estimate was 2 U32 (|mean| rstd |gamma| + |beta|); the code has three roundings on the mean
    path and one on beta.)  For a constant group this is the term that matters: rstd = eps^-1/2 = 316 or 1000 multiplies U32 |mean|.
  * SiLU (`silu_fast`: y * rcp(1 + exp2(-1.4426950408889634f * y))): E_out = 1.1 E_y (max |silu'| = 1.0998) + 6 U32 |silu(y)|
    (v_exp_f32 and v_rcp_f32 one ulp = 2 U32 each, the addition and the product one rounding each) + 2 U32 y^2 sigma (1 - sigma)
    (the rounded constant and the rounded product of the exponent t: d/dt y / (1 + 2^t) = -ln2 y sigma (1 - sigma), |dt| <= 2 U32
    log2e |y|) + |y| 2^-126 (v_rcp_f32 of 1 + 2^t above 2^126, or of an overflowed 2^t = inf, returns zero: sigma below the smallest
    normal f32 is lost, and the product is a signed zero, never a NaN).
LayerNorm (layernorm_rows_kernel, layernorm_kernel, and the copies in rowres.hip's ff_fused_kernel and rowlin_kernel), two-pass:
  * mean.  `sum += v` over the lane's own elements, a shuffle tree, then `sum * invC` (rows form and rowres.hip: invC = 1.0f / C
    rounded, then the product) or `sum / (float)C` (wave form: one correctly rounded division).  As for the GroupNorm partials, no
    operand passes through more than n_l f32 additions, n_l = ln_depth(): the lane's CPL VEC (rows form), MAXS VEC (wave form) or
    160 (rowres.hip, two lanes per row) sequential additions plus the log2(lanes) steps of the tree; C where the form is not given.
    dmean = LAM U32 sqrt(n_l) mean|x| + 2 U32 |mean|.  (The issue expected
    one U32 |mean|; the reciprocal-multiply forms have two roundings.)  It shifts every output by rstd |gamma| dmean and reaches the
    variance only in second order, as dmean^2.
  * variance.  `d = v - mean; sq = fmaf(d, d, sq)`, tree, `sq * invC + eps`: each d carries U32 relative (2 U32 on d^2), the sum
    LAM U32 sqrt(n_l), the scaling 2 U32: dvar = (LAM sqrt(n_l) + 4) U32 var + dmean^2; rstd moves by dvar / (2 (var + eps)) relative,
    plus 3 U32 for `+ eps`, sqrtf and the division `1.0f / sqrtf(..)` -- both correctly rounded: diffsim_amd/build.py's FLAGS carry no
    fast-math option, and in the gfx950 assembly of norm.hip there is no v_rsq_f32 at all and every v_rcp_f32 of the LayerNorm kernels
    sits inside a v_div_scale / v_div_fmas / v_div_fixup sequence (as many v_div_fixup_f32 as v_rcp_f32 in each of them) -- plus eps
    as an f32, U32 eps / (2 (var + eps)).
  * output.  `fmaf(d * rstd, gamma, beta)`: xhat carries 2 U32 (d, the product) and rstd's error; times |gamma|; the fma U32 |y|
    (the issue wrote 2 U32 |ref|; the code has one rounding there).  MOD adds the
    rounding of `1.0f + gamma[..]`: U32 |1 + scale| |xhat|.
Second-order terms (products of two of the errors above, except the two named: rstd_w and dmean^2) are left out.

emulate_*() replay each form's rounding points in float32 on the CPU: the per-thread f32 partials at the kernel's own row striding,
the f64 fold, the casts of mean / rstd, w and sh, the fma, SiLU, the store; the lanes' sequential sums and xor-shuffle trees of the
LayerNorm forms.  They exist so that tests/test_norm64_host.py can hold the REFERENCE ARITHMETIC ALONE to the bound on every case
before any GPU time is spent; they are not bit-exact models (fmas are formed in float64 and rounded once more; the fold order inside
f64 is not replayed)."""
import math

import torch

U = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
U32 = 2.0 ** -24
LAM = 8.0
SILU_DMAX = 1.1                 # max |d/dy y sigma(y)| = 1.0998 (at y = 2.3994)
F16_FLOOR = 2.0 ** -25          # half the spacing of fp16's subnormals
F32_TINY = 2.0 ** -126
GN_THREADS = 256


def vec(dtype):
    return 4 if dtype == torch.float32 else 8


def gn_n_p(plan, HW):
    """rows one thread's f32 partial runs over (the docstring's n_p) for an engine.groupnorm_plan() dict"""
    if plan["form"] == "pre":
        return 256
    if plan["form"] == "onepass":
        return -(-HW // plan["R"])
    return -(-(-(-HW // plan["chunks"])) // plan["R"])


def _out_bound(ref, E, dtype):
    u = U[dtype]
    b = u * ref.abs() + (1 + u) * E
    return b + F16_FLOOR if dtype == torch.float16 else b


def gn_ref_and_bound(x0, x1, gamma, beta, groups, eps, silu, dtype, n_p):
    """x0 [B][HW][C0], x1 None or [B][HW][C1] in the compute dtype; gamma / beta f32 [C].  -> (ref, bound), float64 [B][HW][C]."""
    dev = x0.device
    B, HW = x0.shape[:2]
    g, bt = gamma.to(dev).double(), beta.to(dev).double()
    C = g.numel()
    cpg, n = C // groups, HW * (C // groups)
    ref = torch.empty(B, HW, C, dtype=torch.float64, device=dev)
    bound = torch.empty_like(ref)
    ga, ba = g.abs().view(1, groups, cpg), bt.abs().view(1, groups, cpg)
    acc = LAM * U32 * math.sqrt(n_p)
    for b in range(B):                                          # one image at a time: the 33 M-element maps fit a GPU's memory
        x = (x0[b].double() if x1 is None else torch.cat([x0[b].double(), x1[b].double()], 1)).view(HW, groups, cpg)
        mean = x.mean((0, 2), keepdim=True)
        d = x - mean
        var = (d * d).mean((0, 2), keepdim=True)
        rstd = (var + eps).rsqrt()
        y = d * rstd * g.view(1, groups, cpg) + bt.view(1, groups, cpg)
        dmean = acc * x.abs().sum((0, 2), keepdim=True) / n
        dvar = acc * (x * x).sum((0, 2), keepdim=True) / n + 2 * mean.abs() * dmean
        rw = ((var - dvar).clamp_min(0) + eps).rsqrt()
        E = ga * (rw * dmean + d.abs() * rw ** 3 * dvar / 2)                                   # statistics
        E = E + d.abs() * rstd * ga * (U32 * eps / (2 * (var + eps)))                           # eps as an f32
        E = E + U32 * (2 * d.abs() * rstd * ga + 3 * mean.abs() * rstd * ga + ba + y.abs())     # affine
        if silu:
            sg = torch.sigmoid(y)
            r = y * sg
            E = SILU_DMAX * E + 6 * U32 * r.abs() + 2 * U32 * y * y * sg * (1 - sg) + y.abs() * F32_TINY
        else:
            r = y
        ref[b] = r.view(HW, C)
        bound[b] = _out_bound(r, E, dtype).view(HW, C)
    return ref, bound


def ln_depth(plan, dtype):
    """f32 additions an operand passes through (the docstring's n_l) for an engine.layernorm_plan() dict, or dict(form="rowres")"""
    if plan["form"] == "rows":
        return plan["CPL"] * vec(dtype) + int(math.log2(plan["LPR"]))
    if plan["form"] == "wave":
        return plan["MAXS"] * vec(dtype) + 6
    return 160 + 1


def ln_ref_and_bound(x, gamma, beta, eps, dtype, rows_per_batch=0, depth=None):
    """x [M][C] in the compute dtype.  rows_per_batch = 0: affine LayerNorm, gamma / beta f32 [C]; > 0: the modulated form, gamma =
    scale2, beta = shift2, f32 [2][C].  depth: ln_depth() of the form that ran (None: C).  -> (ref, bound), float64 [M][C]."""
    dev = x.device
    M, C = x.shape
    n_l = C if depth is None else depth
    ref = torch.empty(M, C, dtype=torch.float64, device=dev)
    bound = torch.empty_like(ref)
    g, bt = gamma.to(dev).double(), beta.to(dev).double()
    for r0 in range(0, M, 1 << 16):
        xs = x[r0:r0 + (1 << 16)].double()
        if rows_per_batch:
            half = ((torch.arange(r0, r0 + xs.shape[0], device=dev) // rows_per_batch) & 1)
            gg, bb = 1.0 + g.view(2, C)[half], bt.view(2, C)[half]
        else:
            gg, bb = g.view(1, C), bt.view(1, C)
        mean = xs.mean(1, keepdim=True)
        d = xs - mean
        var = (d * d).mean(1, keepdim=True)
        rstd = (var + eps).rsqrt()
        xhat = d * rstd
        y = xhat * gg + bb
        dmean = LAM * U32 * math.sqrt(n_l) * xs.abs().mean(1, keepdim=True) + 2 * U32 * mean.abs()
        dvar = (LAM * math.sqrt(n_l) + 4) * U32 * var + dmean * dmean
        rel = dvar / (2 * (var + eps)) + 3 * U32 + U32 * eps / (2 * (var + eps))
        dx = xhat.abs() * (2 * U32 + rel) + rstd * dmean
        E = gg.abs() * dx + U32 * y.abs()
        if rows_per_batch:
            E = E + U32 * gg.abs() * xhat.abs()
        ref[r0:r0 + xs.shape[0]] = y
        bound[r0:r0 + xs.shape[0]] = _out_bound(y, E, dtype)
    return ref, bound


def excess(got, ref, bound):
    """largest |got - ref| / bound over all elements; inf if any element of got is not finite"""
    g = got.to(ref.device).double().reshape(ref.shape)
    if not torch.isfinite(g).all():
        return float("inf")
    return float(((g - ref).abs() / bound.clamp_min(1e-300)).max())


def check(got, ref, bound, what=""):
    """Returns the largest err / bound; raises with the worst element on any violation."""
    g = got.to(ref.device).double().reshape(ref.shape)
    assert torch.isfinite(g).all(), f"{what}: non-finite output"
    ratio = (g - ref).abs() / bound.clamp_min(1e-300)
    worst = float(ratio.max())
    if worst > 1.0:
        i = int(ratio.argmax())
        idx = []
        for s in reversed(ref.shape):
            idx.append(i % s)
            i //= s
        idx = tuple(reversed(idx))
        raise AssertionError(f"{what}: {int((ratio > 1).sum())} elements out of bound; worst at {idx}: got {float(g[idx]):.9g} "
                             f"ref {float(ref[idx]):.9g} bound {float(bound[idx]):.3g} (err / bound {worst:.3f})")
    return worst


# ---- float32 replays of the kernels' rounding points (CPU) ---------------------------------------------------------------------
def _fma32(a, b, c):
    """fmaf on float32 tensors: the product is exact in float64; one extra rounding (f64 sum, then f32)"""
    return (a.double() * b.double() + c.double()).float()


def _seq_sums(rows):
    """rows [..., n_p, W] float32, zero where a thread has no row: running f32 sums and fma sums of squares in row order"""
    s1 = torch.zeros(rows.shape[:-2] + rows.shape[-1:], dtype=torch.float32)
    s2 = torch.zeros_like(s1)
    for i in range(rows.shape[-2]):
        f = rows[..., i, :]
        s1 = s1 + f
        s2 = _fma32(f, f, s2)
    return s1, s2


def gn_partials(x, plan):
    """(S1, S2) float64, per channel [C] (pre: per 4-channel quad [C / 4]), of one image x [HW][C] float32: every thread's f32
    partials at the kernel's row striding (rows r0 + trow, + R, ... of each slab), summed in float64 as the folds do."""
    HW, C = x.shape
    R = plan["R"]
    if plan["form"] == "pre":           # one f32 (sum, sumsq) per 64 rows x 4 channels, as a conv epilogue leaves them: here rounded sums
        q = x.double().view(HW // 64, 64, C // 4, 4)
        s1 = q.sum((1, 3)).float().double().sum(0)
        s2 = (q * q).sum((1, 3)).float().double().sum(0)
        return s1, s2
    chunks = plan["chunks"] if plan["form"] == "twopass" else 1
    n_p = gn_n_p(plan, HW)
    idx = torch.full((chunks, R, n_p), HW, dtype=torch.int64)
    for c in range(chunks):
        r0, r1 = HW * c // chunks, HW * (c + 1) // chunks
        for t in range(R):
            if r0 + t < r1:
                rows = torch.arange(r0 + t, r1, R)
                idx[c, t, :len(rows)] = rows
    xz = torch.cat([x, torch.zeros(1, C)], 0)
    s1, s2 = _seq_sums(xz[idx])                                   # [chunks][R][C]
    return s1.double().sum((0, 1)), s2.double().sum((0, 1))


def silu_fast32(y):
    t = (torch.tensor(-1.4426950408889634, dtype=torch.float32) * y)
    return y * (1.0 / (1.0 + torch.exp2(t)))


def emulate_groupnorm(x0, x1, gamma, beta, groups, eps, silu, dtype, plan):
    """the GroupNorm forms replayed in float32 (see the module docstring) -> [B][HW][C] in dtype"""
    x = (x0 if x1 is None else torch.cat([x0, x1], 2)).cpu().float()
    B, HW, C = x.shape
    cpg = C // groups
    g32, b32 = gamma.cpu().float(), beta.cpu().float()
    epsd = float(torch.tensor(eps, dtype=torch.float32))
    out = torch.empty(B, HW, C, dtype=dtype)
    for b in range(B):
        s1, s2 = gn_partials(x[b], plan)
        a, q = s1.view(groups, -1).sum(1), s2.view(groups, -1).sum(1)
        n = float(HW * cpg)
        mean = a / n
        var = (q / n - mean * mean).clamp_min(0)
        mean32 = mean.float().repeat_interleave(cpg)
        rstd32 = (1.0 / torch.sqrt(var + epsd)).float().repeat_interleave(cpg)
        w = g32 * rstd32
        sh = b32 - mean32 * w
        y = _fma32(x[b], w.view(1, C), sh.view(1, C))
        out[b] = (silu_fast32(y) if silu else y).to(dtype)
    return out


def _tree(p):
    """xor-shuffle butterfly over the last dimension (a power of two): every lane ends with the same f32 sum; lane 0's returned"""
    n = p.shape[-1]
    off = n // 2
    lanes = torch.arange(n)
    while off:
        p = p + p[..., lanes ^ off]
        off //= 2
    return p[..., 0]


def _ln_lanes(x, plan, dtype):
    """x [M][C] float32 -> [M][lanes][elements per lane] in each lane's own order, zero-padded"""
    M, C = x.shape
    V = vec(dtype)
    S = C // V
    ch = x.view(M, S, V)
    if plan["form"] == "rows":
        L, CPL = plan["LPR"], plan["CPL"]
        return ch.view(M, CPL, L, V).permute(0, 2, 1, 3).reshape(M, L, CPL * V)       # lane s: chunks s, s + LPR, ...
    if plan["form"] == "wave":
        K = plan["MAXS"]
        pad = torch.zeros(M, 64 * K, V)
        pad[:, :S] = ch
        return pad.view(M, K, 64, V).permute(0, 2, 1, 3).reshape(M, 64, K * V)        # lane l: chunks l, l + 64, ...
    assert plan["form"] == "rowres" and V == 8                                         # lane `half`: channels 16 ks + 8 half ...
    return ch.view(M, S // 2, 2, V).permute(0, 2, 1, 3).reshape(M, 2, (S // 2) * V)


def emulate_layernorm(x, gamma, beta, eps, dtype, plan, rows_per_batch=0):
    """the LayerNorm forms replayed in float32: plan from engine.layernorm_plan(), or dict(form="rowres") for rowres.hip's copies
    (two lanes per row, 160 channels each at C = 320) -> [M][C] in dtype"""
    xf = x.cpu().float()
    M, C = xf.shape
    lanes = _ln_lanes(xf, plan, dtype)
    valid = _ln_lanes(torch.ones(1, C), plan, dtype)[0] > 0
    eps32 = torch.tensor(eps, dtype=torch.float32)
    s = torch.zeros(lanes.shape[:2])
    for i in range(lanes.shape[2]):
        s = s + lanes[:, :, i]
    tot = _tree(s)
    if plan["form"] == "wave":
        mean = tot / torch.tensor(float(C), dtype=torch.float32)
    else:
        invC = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(C), dtype=torch.float32)
        mean = tot * invC
    sq = torch.zeros_like(s)
    for i in range(lanes.shape[2]):
        d = (lanes[:, :, i] - mean.view(M, 1)) * valid[:, i].float()
        sq = _fma32(d, d, sq)
    tsq = _tree(sq)
    v = tsq / torch.tensor(float(C), dtype=torch.float32) if plan["form"] == "wave" else tsq * invC
    rstd = 1.0 / torch.sqrt(v + eps32)
    xhat = (xf - mean.view(M, 1)) * rstd.view(M, 1)
    g32, b32 = gamma.cpu().float(), beta.cpu().float()
    if rows_per_batch:
        half = (torch.arange(M) // rows_per_batch) & 1
        gg, bb = 1.0 + g32.view(2, C)[half], b32.view(2, C)[half]
    else:
        gg, bb = g32.view(1, C), b32.view(1, C)
    return _fma32(xhat, gg, bb).to(dtype)
