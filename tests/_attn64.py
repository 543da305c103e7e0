"""A float64 restatement of scaled-dot-product attention (every kernel attention_kernel() in csrc/attention.hip picks, on the tiled
core of csrc/attn_core.h, sdpa160_kernel in csrc/attn160.hip and attn_fp8_kernel in csrc/attention_fp8.hip) and its per-element error
bound, shared by the attention tests.  Not a conftest: import it like tests/_gemm64.py.

The semantics are the models': O = softmax(q k^T / sqrt(D)) v per (batch element, head), batch element b reading K / V element b % Bkv.
Operands are taken as the kernel sees them: q, k, v in the compute dtype (bf16 / fp16 / f32), as float64.  The reference is
tests/_tail64.sdpa64 on the device the tensors live on, in query chunks.  Logits are written in log2 units, t_j = c q.k_j with
c = log2(e) / sqrt(D) (the kernels' scale_log2), weights w_j = 2^(t_j - max t) / sum, and R_jd = v_jd - O_d.

THE BOUND.  Per element (query row, column d):

    |got - ref| <= u_out |ref|  +  (1 + u_out) E,    E = T_q + T_s + T_k + T_p + T_floor + T_v + T_acc + T_div

  * u_out: the output store's rounding (2^-24 f32, 2^-8 bf16, 2^-11 fp16), applied to the kernel's value, which is ref + E; fp16
    adds 2^-25 absolute (OUT_FLOOR: half its subnormal spacing, for outputs below 2^-14).
  * T_q, the rounding of the pre-scaled Q: the tiled kernels load Q as round(c q) in the compute type (attn_core.h load_q /
    gload_frag_scaled; fp8: e4m3, attn_fp8_kernel's chunk_to_fp8 of the Q row).  A relative error delta_p of element p moves
    every logit t_j by delta_p c q_p k_jp, so the output by ln2 sum_p delta_p c q_p G_pd, G_pd = sum_j w_j k_jp R_jd -- one
    deterministic term per element: T_q = ln2 sum_p err_q(c q_p) |G_pd|, err_q(x) = max(u_q |x|, the type's subnormal floor).  The
    short-key kernel (attn_short_kernel, exp2(fma(s, c, -m c)) on raw logits, its load_q_raw) and sdpa160_kernel
    (exp2(fmaf(s, c, mc))) do NOT round Q: u_q = 0 there.
  * T_s, the logit's f32 arithmetic: the QK^T accumulation, which in the tiled kernels starts at -m (attend: minit, the
    accumulators' start value; KONE, D = 8 mod 16: -m rides in Q's spare column as an exactly representable h16, attend's m_new),
    so it is relative to c sum_p |q_p k_jp| + |m|: lam u32 sqrt(D + 1) of that; the exp2 (v_exp_f32, one ulp: 2 u32 / ln2 in log2
    units); the subtraction of the reference, the fma and the scale constant's own f32 rounding: 4 u32 (|t_j| + |t_max|).  Its
    effect is ln2 sum_j w_j e_j |R_jd|.
  * T_k, T_v (fp8 only): K and V rounded to e4m3 per element (chunk_to_fp8 where attn_fp8_kernel stages a tile): independent,
    mean-zero errors, so
    lam ln2 sqrt(sum_j w_j^2 R_jd^2 sum_p (c q_p err8(k_jp))^2) and lam sqrt(sum_j w_j^2 err8(v_jd)^2).
  * T_p, P rounded to the MFMA operand type before PV (attend: the pf fragments; attend2, attend_pipelined2, the short
    kernel and attn160.hip's three kernels alike; fp8: pack4_fp8 into plo / phi).  Where the row sum l adds the
    ROUNDED P -- the ones column of V (ACfg::ONES: D in {16, 40, 72, 80}) or the ones row of V^T (fp8) -- the rounding is a
    reweighting and moves O by sum_j w_j delta_j R_jd: lam u_P sqrt(sum_j w_j^2 R_jd^2).  Where l adds the unrounded f32 P (D = 32,
    64, 160: the `if constexpr (!C::ONES)` branch of attend; sdpa160_kernel's psum) the numerator alone moves:
    lam u_P sqrt(sum_j w_j^2 v_jd^2).  P may exceed 1 under the fixed-reference softmax (tile 0's maximum: up to DSIM_H16_LSUM_MAX =
    3e4 in fp16 before attend_checked's fallback) and under sdpa160's 8-unit rescale threshold: the error is relative all
    the same.  f32 has no rounding here (u_P = 0).
  * T_floor: fp16's subnormal P (below 2^-14) is rounded with an absolute error up to 2^-25; the row sum in the kernel's frame is
    >= 1/2 (the row maximum's own P is ~1, attend_checked takes anything below 1/4 for a fault), so per key 2^-24 of weight:
    lam 2^-24 sqrt(sum_j R_jd^2).  fp8's P = p 2^7 (attn_fp8_kernel's PSH) below e4m3's 2^-6 carries 2^-10 absolute against
    l >= 64: lam 2^-16 sqrt(sum_j R_jd^2).
  * T_acc: the f32 PV and row-sum accumulations over Nk products plus one rescale per key tile (attend's alpha):
    lam u32 sqrt(Nk + Nk / 64 + 2) (sum_j w_j |v_jd| + |O_d|).
  * T_div: 1 / l and the product (attend's inv; sdpa160's v_rcp_f32): 3 u32 |O_d|.
lam = LAM = 8 as in tests/_gemm64.py (Higham and Mary, SIAM J. Sci. Comput. 41(5), 2019, Theorem 3.1): independent, mean-zero
rounding errors sum to at most lam sqrt(n) u of their magnitudes with probability >= 1 - 2n exp(-lam^2 / 2).  It is chosen from that
statement, not fitted to the kernels.  Second-order terms (products of two roundings, ~1e-6 relative to E) are left out.

emulate() replays each kind's rounding points in float32 on the CPU (pre-scaled or raw Q, -m in the accumulator, the tile-wise
running or fixed reference, KONE's rounded maximum, P rounded to the operand type, which P the row sum adds, the output rounding):
the host tests hold it to the bound and check that the bound rejects the perturbed forms a kernel bug would produce.
"""
import math

import torch

from tests._tail64 import sdpa64

U = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
U32 = 2.0 ** -24
U8 = 2.0 ** -4                  # e4m3: 3 mantissa bits, round to nearest even
LAM = 8.0
LN2 = math.log(2.0)
KT = 64                         # key rows per tile of the tiled kernels
BUDGET = 1 << 23                # float64 elements of a chunk's [groups][rows][Nk][D] tensors
F16_LSUM_MAX = 3.0e4            # common.h DSIM_H16_LSUM_MAX (fp16)
OUT_FLOOR = {torch.float32: 0.0, torch.bfloat16: 0.0, torch.float16: 2.0 ** -25}     # absolute rounding error of a subnormal output

KINDS = ("P160", "Short", "ShortK80", "Long", "Q2", "Q2Fast", "Fast", "Exact", "FP8")     # dsim_attn_kind order
FAST_KINDS = ("Long", "Q2Fast", "Fast")
RAW_Q_KINDS = ("P160", "Short", "ShortK80")


def scale_log2(D):
    """the kernels' c = log2(e) / sqrt(D), as scale_log2_of computes it in f32"""
    c = torch.tensor(1.0, dtype=torch.float32) / torch.sqrt(torch.tensor(float(D), dtype=torch.float32))
    return float(c * torch.tensor(1.4426950408889634, dtype=torch.float32))


def ones_sum(kind, D):
    """does the row sum add the ROUNDED P (a ones column of V / ones row of V^T)?"""
    if kind == "FP8":
        return True
    if kind == "P160":
        return False
    return D % 32 != 0 and D < 160                  # ACfg::ONES: D < NDB * 32


class Spec:
    """the rounding points of one (kind, dtype, D)"""

    def __init__(self, kind, dtype, D):
        assert kind in KINDS, kind
        self.kind, self.dtype, self.D = kind, dtype, D
        f8 = kind == "FP8"
        self.u_out = U[dtype]
        self.out_floor = OUT_FLOOR[dtype]
        self.u_q = 0.0 if kind in RAW_Q_KINDS else (U8 if f8 else U[dtype]) + U32
        self.q_floor = 2.0 ** -10 if f8 else (2.0 ** -25 if dtype == torch.float16 else 0.0)
        self.u_kv = U8 if f8 else 0.0
        self.u_p = U8 if f8 else (0.0 if dtype == torch.float32 else U[dtype])
        self.p_floor = 2.0 ** -16 if f8 else (2.0 ** -24 if dtype == torch.float16 else 0.0)
        self.ones = ones_sum(kind, D)
        self.m_in_acc = kind not in RAW_Q_KINDS


def _err8(x):
    return torch.clamp(U8 * x.abs(), min=2.0 ** -10)


def _row_chunks(G, Nq, per_row):
    """(g0, g1, r0, r1) pieces of a [G][Nq] row set whose [g][r][per_row] float64 tensors stay within BUDGET"""
    rows = max(1, BUDGET // max(per_row, 1))
    if rows >= Nq:
        gs = max(1, rows // Nq)
        for g0 in range(0, G, gs):
            yield g0, min(G, g0 + gs), 0, Nq
    else:
        for g0 in range(G):
            for r0 in range(0, Nq, rows):
                yield g0, g0 + 1, r0, min(Nq, r0 + rows)


@torch.no_grad()
def ref_and_bound(q, k, v, spec):
    """q [G][Nq][D], k / v [G][Nk][D] float64 (the operands as the kernel sees them; any device).  Returns (ref, bound), each
    [G][Nq][D] float64 on that device."""
    G, Nq, D = q.shape
    Nk = k.shape[1]
    ref = sdpa64(q.unsqueeze(0), k.unsqueeze(0), v.unsqueeze(0))[0]
    c = math.log2(math.e) / math.sqrt(D)
    bound = torch.empty_like(ref)
    for g0, g1, r0, r1 in _row_chunks(G, Nq, Nk * D * 3):
        Q, K, V = q[g0:g1, r0:r1], k[g0:g1], v[g0:g1]
        O = ref[g0:g1, r0:r1]
        t = c * torch.matmul(Q, K.transpose(1, 2))                       # [g][r][Nk] log2 units
        tmax = t.amax(-1, keepdim=True)
        w = torch.exp2(t - tmax)
        w = w / w.sum(-1, keepdim=True)
        R = V.unsqueeze(1) - O.unsqueeze(2)                               # [g][r][Nk][D]
        absqk = c * torch.matmul(Q.abs(), K.abs().transpose(1, 2))
        e = LAM * U32 * math.sqrt(D + 1) * (absqk + (tmax.abs() if spec.m_in_acc else 0.0)) + \
            4 * U32 * (t.abs() + tmax.abs()) + 2 * U32 / LN2
        E = LN2 * torch.einsum("grj,grjd->grd", w * e, R.abs())
        if spec.u_q:
            Gm = torch.einsum("grj,gjp,grjd->grpd", w, K, R)
            cq = c * Q.abs()
            eq = torch.clamp(spec.u_q * cq, min=spec.q_floor)
            E += LN2 * torch.einsum("grp,grpd->grd", eq, Gm.abs())
        w2 = w * w
        if spec.u_kv:
            a = w2 * torch.matmul((c * Q) ** 2, (_err8(K) ** 2).transpose(1, 2))
            E += LN2 * LAM * torch.einsum("grj,grjd->grd", a, R * R).sqrt()
            E += LAM * torch.matmul(w2, _err8(V) ** 2).sqrt()
        if spec.u_p:
            if spec.ones:
                E += LAM * spec.u_p * torch.einsum("grj,grjd->grd", w2, R * R).sqrt()
            else:
                E += LAM * spec.u_p * torch.matmul(w2, V * V).sqrt()
        if spec.p_floor:
            E += LAM * spec.p_floor * (R * R).sum(2).sqrt()
        E += LAM * U32 * math.sqrt(Nk + Nk / KT + 2) * (torch.matmul(w, V.abs()) + O.abs()) + 3 * U32 * O.abs()
        bound[g0:g1, r0:r1] = spec.u_out * O.abs() + spec.out_floor + (1 + spec.u_out) * E
    return ref, bound


def excess(got, ref, bound):
    """max over elements of |got - ref| / bound (non-finite got counts as infinite)"""
    err = (got.double() - ref).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, math.inf))
    return float((err / bound).max())


# ---- emulation of the kernels' rounding points (float32, CPU) ---------------------------------------------------------------
def _rnd(x, dtype):
    return x if dtype == torch.float32 else x.to(dtype).float()


def _e4m3(x):
    return x.to(torch.float8_e4m3fn).float()


def _f32(x64):
    return x64.float()


@torch.no_grad()
def emulate(q, k, v, kind, dtype):
    """the kernel `kind` in `dtype`, rounding point by rounding point: q [G][Nq][D], k / v [G][Nk][D] (values of the compute dtype,
    any float type).  Returns [G][Nq][D] float64 (the stored output)."""
    G, Nq, D = q.shape
    Nk = k.shape[1]
    c = scale_log2(D)
    q32, k32, v32 = q.float(), k.float(), v.float()
    f8 = kind == "FP8"
    ones = ones_sum(kind, D)
    prnd = _e4m3 if f8 else (lambda x: _rnd(x, dtype))
    if kind in RAW_Q_KINDS:
        s = torch.matmul(q32, k32.transpose(1, 2))                       # raw logits, f32
        m = s.amax(-1, keepdim=True)
        t = _f32(s.double() * c - (m * c).double())                      # fma(s, c, -m c): one rounding
        P = torch.exp2(t)
        Pr = prnd(P)
        O = torch.matmul(Pr, v32)
        l = (Pr if ones else P).sum(-1, keepdim=True)
        return _rnd(O * (1.0 / l), dtype).double()
    if f8:
        qs, k32, v32 = _e4m3(q32 * c), _e4m3(k32), _e4m3(v32)
    else:
        qs = _rnd(q32 * c, dtype)
    kone = dtype != torch.float32 and not f8 and D % 16 == 8
    shift = 7.0 if f8 else 0.0

    def run(fast):
        O = torch.zeros(G, Nq, D)
        l = torch.zeros(G, Nq, 1)
        m = torch.zeros(G, Nq, 1)
        for j0 in range(0, Nk, KT):
            kt, vt = k32[:, j0:j0 + KT], v32[:, j0:j0 + KT]
            s = torch.matmul(qs, kt.transpose(1, 2)) - m                  # the accumulators start at -m
            tmax = s.amax(-1, keepdim=True)
            if j0 == 0 or (not fast and bool((tmax > shift).any())):
                delta = tmax - shift if j0 == 0 else torch.clamp(tmax - shift, min=0.0)
                if kone:
                    m_new = _rnd(m + delta, dtype)
                    delta = m_new - m
                    m = m_new
                else:
                    m = m + delta
                s = s - delta
                if j0:
                    alpha = torch.exp2(-delta)
                    O, l = O * alpha, l * alpha
            P = torch.exp2(s)
            Pr = prnd(P)
            O = O + torch.matmul(Pr, vt)
            l = l + (Pr if ones else P).sum(-1, keepdim=True)
        return O, l

    fast = kind in FAST_KINDS
    O, l = run(fast)
    if fast:
        lim = F16_LSUM_MAX if dtype == torch.float16 else 1e30
        bad = ~((l > 0.25) & (l < lim))
        if bool(bad.any()):
            O2, l2 = run(False)
            O = torch.where(bad, O2, O)
            l = torch.where(bad, l2, l)
    return _rnd(O * (1.0 / l), dtype).double()


def heads(t, Bn, N, H, D):
    """[Bn][N][H*D] (or rows of a wider ld, already sliced) -> [Bn*H][N][D]"""
    return t.reshape(Bn, N, H, D).transpose(1, 2).reshape(Bn * H, N, D)


def expand_kv(kh, B, Bkv, H):
    """[Bkv*H][Nk][D] -> [B*H][Nk][D]: batch element b reads K / V element b % Bkv"""
    Nk, D = kh.shape[1:]
    idx = torch.arange(B, device=kh.device) % Bkv
    return kh.reshape(Bkv, H, Nk, D)[idx].reshape(B * H, Nk, D)


def softmax_rows_bound(x, scale, dtype):
    """(ref, bound) of softmax_rows_kernel (csrc/norm.hip): out = softmax(x * scale) per row, x [rows][cols] float64 values of the
    compute dtype.  The kernel computes exp2(fmaf(x, c, -m c)) in f32 (c = scale log2(e): one f32 rounding of the constant, one of the
    fma, exp2f's few ulps), sums the row in f32 and multiplies by 1 / sum: per element
      |got - ref| <= u_out ref + (1 + u_out) ref (ln2 (4 u32 (|t| + |t_max|) + 4 u32 / ln2) + lam u32 sqrt(cols) + 3 u32 + mean term)
    with the mean term ln2 sum_j w_j 4 u32 (|t_j| + |t_max|) for the denominator's share of the same errors, plus OUT_FLOOR for
    fp16's subnormal outputs (weights below 2^-14 are common: a 784-column row's smallest)."""
    c = scale * math.log2(math.e)
    t = x * c
    tmax = t.amax(-1, keepdim=True)
    w = torch.exp2(t - tmax)
    w = w / w.sum(-1, keepdim=True)
    et = 4 * U32 * (t.abs() + tmax.abs()) + 4 * U32 / LN2
    rel = LN2 * (et + (w * et).sum(-1, keepdim=True)) + LAM * U32 * math.sqrt(x.shape[-1]) + 3 * U32
    u = U[dtype]
    return w, u * w + OUT_FLOOR[dtype] + (1 + u) * w * rel
