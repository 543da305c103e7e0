"""Text attention maps and text-guided regions (csrc/textattn.hip: text_attn_kernel + text_region_kernel behind
dsim_text_attention) restated in float64, with a per-entry bound on the kernels' f32 arithmetic, shared by
tests/test_textattn_host.py, tests/test_gpu_textattn.py and tests/test_gpu_text_regions.py.  Not a conftest: import it like
tests/_align64.py.

THE DEFINITION.  With the operands as stored (xq [n][2][N][H*D], xkv [n_kv][L][2*H*D] in the compute dtype, K in the first H*D
columns; every 16-bit value is exact in float64), for image i on the conditional CFG half (batch element e = 2 i + 1; context row 1
when n_kv == 2, row e when n_kv == 2 n):
    P_h[n][l] = softmax_l(xq_h[n,:] . xk_h[l,:] / sqrt(D)),      T[n][l] = mean over the H heads of P_h[n][l]
    s[n] = sum_l w[l] T[n][l],      m = mean_n s[n],      token n on iff s[n] >= rel_threshold * m;  no token on -> every token on.

THE BOUND on T, term by term as tests/_align64.py builds its own (same arithmetic: align_logits, exp2(fma(s, c, -m c)); u32 = 2^-24,
first order; t = logit in natural units, gap_nl = max_l t_nl - t_nl >= 0, p = P_h).  Nothing is rounded to 16 bits, so the bound
does not depend on the compute dtype.
  * the f32 accumulation of exact products on the MFMAs: a_nl = LAM u32 sqrt(D) (|Q| |K|^T)_nl / sqrt(D), LAM = 8 (_gemm64).  The row
    maximum is the maximum of the computed logits and cancels between a probability and its denominator: no term.
  * the f32 scale: arg = fma(s, c, -m c), c rounded to f32 and the fma rounded: 2 u32 gap_nl in natural units.
  * exp2 at hardware accuracy, 2^-23 relative; flushed arguments: an absolute floor of 2^-124 per entry.
    Together the numerator has relative error rho_nl = a_nl + 2 u32 gap_nl + 2^-23.
  * the f32 denominator and reciprocal.  l = sum_l e_nl carries sum_l p_nl rho_nl; the sum itself is ONE pass over the whole key set
    (L <= 128: no tiles, no rescale): 64 slots per lane half added in turn and the add of the two halves, a sum of non-negative
    terms: 64 u32 l at worst; 1 / l one correctly rounded division, counted as 2 u32:
        den_n = sum_l p_nl rho_nl + 66 u32
  * the f32 head sum.  acc = fma(e, 1 / l, acc) over the H heads ascending: one rounding per step of a partial sum that never exceeds
    H T: H u32 relative to T after the mean; the factor 1 / H rounded once and multiplied once: 2 u32.
        bound_nl = mean_h p_nl (rho_nl + den_n) + (H + 2) u32 T_nl + 2^-124
No constant is fitted to what the kernels return.

THE GATES.  attn: the project's per-op gate ORDINARY_REL x the reference row's maximum on the ordinary family (q scaled by 1), the
bound above on the scaled family (q scaled by 3), as tests/test_gpu_align.py.  saliency: sum_l |w_l| gate_nl plus the fma chain's
own rounding, (L + 1) u32 sum_l |w_l| T_nl.  mask: equal to the float64 mask on every token outside the band |s - thr m| <= the
token's saliency gate + thr x the image's largest saliency gate (the mean moves by at most that); at most BAND_SHARE of a case's
tokens may lie inside (a condition on the inputs, checked on the CPU by tests/test_textattn_host.py).

THE FAMILIES.  operands(): seeded randn, q scaled by 1 ("ordinary") or 3 ("scaled"); weights(): 1 on tokens 5-7, on tokens 1-3
when L = 13, on token 0 when L = 1.  planted(): unit-scale random K, a seeded token set S of about N / 4 whose queries are
gain k[l*] in every head, all others gain k[l0]; w = one-hot l*."""
import math

import torch

from tests import _gemm64 as G

U32, LAM = G.U32, G.LAM
EXP2_REL = 2.0 ** -23
FLOOR = 2.0 ** -124
ORDINARY_REL = 2e-5                               # the project's per-op gate, relative to the reference row's maximum
BAND_SHARE = 0.02                                 # at most this share of a case's tokens may sit inside the threshold band
FAMILIES = {"ordinary": 1.0, "scaled": 3.0}
ALL3 = (torch.bfloat16, torch.float16, torch.float32)
H16 = (torch.bfloat16, torch.float16)
# (N, H, D, L) -> dtypes of the cases of tests/test_gpu_textattn.py
SHAPES = {(49, 2, 16, 13): ALL3,        # ragged wave; TINY's context length
          (81, 4, 40, 77): ALL3,        # d padded 40 -> 48; L = 2 blocks + 13
          (64, 20, 64, 77): H16,        # SDXL heads
          (256, 8, 160, 77): ALL3,      # the default tap; the f32 tile through dynamic LDS
          (1024, 8, 80, 33): H16,       # one key past a 32-block; many query tiles
          (70, 1, 32, 128): ALL3,       # the maximum L
          (33, 3, 72, 1): ALL3}         # L = 1: T == 1 exactly
N_IMAGES = 3
PLANTED = ((49, 2, 16, 13), (81, 4, 40, 77), (256, 8, 160, 77), (70, 1, 32, 128))


def operands(n, seed, dtype, N, H, D, L, q_scale=1.0, n_kv=None):
    """xq [n][2][N][H*D], xkv [n_kv][L][2*H*D] on the CPU in dtype; n_kv None: a context per batch element (2 n)"""
    g = torch.Generator().manual_seed(seed)
    xq = (torch.randn(n, 2, N, H * D, generator=g) * q_scale).to(dtype).contiguous()
    xkv = torch.randn(2 * n if n_kv is None else n_kv, L, 2 * H * D, generator=g).to(dtype).contiguous()
    return xq, xkv


def weights(L):
    w = torch.zeros(L)
    if L == 1:
        w[0] = 1.0
    elif L == 13:
        w[1:4] = 1.0
    else:
        w[5:8] = 1.0
    return w


def _heads(t, H):
    """[R][H*D] -> float64 [H][R][D]"""
    R, HD = t.shape
    return t.double().view(R, H, HD // H).permute(1, 0, 2)


def image64(xq_i, xk_i, H, with_bound=True):
    """(T, bound) [N][L] float64 of one image: xq_i [N][H*D] its conditional half's queries, xk_i [L][H*D] its cond keys"""
    Q, K = _heads(xq_i, H), _heads(xk_i, H)
    D = Q.shape[-1]
    t = Q @ K.transpose(1, 2) / math.sqrt(D)
    P = torch.softmax(t, -1)
    T = P.mean(0)
    if not with_bound:
        return T, None
    a = (Q.abs() @ K.abs().transpose(1, 2)) * (LAM * U32 * math.sqrt(D) / math.sqrt(D))
    gap = t.max(-1, keepdim=True).values - t
    rho = a + 2 * U32 * gap + EXP2_REL
    den = (P * rho).sum(-1, keepdim=True) + 66 * U32
    bound = (P * (rho + den)).mean(0) + (H + 2) * U32 * T + FLOOR
    return T, bound


def attn64(xq, xkv, H, with_bound=True):
    """(T, bound): float64 [n][N][L] each (bound None without with_bound)"""
    n, C = xq.shape[0], xq.shape[3]
    n_kv = xkv.shape[0]
    rows = [image64(xq[i, 1], xkv[1 if n_kv == 2 else 2 * i + 1][:, :C], H, with_bound) for i in range(n)]
    return torch.stack([r[0] for r in rows]), (torch.stack([r[1] for r in rows]) if with_bound else None)


def attn_gate(T, bound, family):
    return ORDINARY_REL * T.max(-1, keepdim=True).values.expand_as(T) if family == "ordinary" else bound


def saliency64(T, w):
    """s [n][N] float64: w (L,) shared or (n, L) per image"""
    w = w.double()
    return (T * (w[None, None] if w.ndim == 1 else w[:, None])).sum(-1)


def saliency_gate(T, gate, w):
    w = w.double().abs()
    wb = w[None, None] if w.ndim == 1 else w[:, None]
    L = T.shape[-1]
    return (wb * gate).sum(-1) + (L + 1) * U32 * (wb * T).sum(-1)


def region64(s, thr=1.0):
    """(mask bool [n][N], counts [n], m [n]) of float64 saliency: on iff s >= thr m; nothing on -> everything on"""
    m = s.mean(-1)
    on = s >= thr * m[:, None]
    on[~on.any(-1)] = True
    return on, on.sum(-1), m


def band(s, sgate, thr=1.0):
    """bool [n][N]: the tokens whose side of the threshold the kernel's f32 saliency and f64 mean may not settle"""
    m = s.mean(-1, keepdim=True)
    return (s - thr * m).abs() <= sgate + thr * sgate.max(-1, keepdim=True).values


def planted(seed, dtype, N, H, D, L, gain):
    """(xq [1][2][N][H*D], xkv [2][L][2*H*D], w one-hot l*, S bool [N]): the queries of S point at key l* in every head, all
    others at key l0"""
    g = torch.Generator().manual_seed(seed)
    xkv = torch.randn(2, L, 2 * H * D, generator=g)
    S = torch.zeros(N, dtype=torch.bool)
    S[torch.randperm(N, generator=g)[:max(1, N // 4)]] = True
    lstar, l0 = (L // 2, 0) if L > 1 else (0, 0)
    k = xkv[1, :, :H * D]
    xq = torch.empty(1, 2, N, H * D)
    xq[0, :, S] = gain * k[lstar]
    xq[0, :, ~S] = gain * k[l0]
    w = torch.zeros(L)
    w[lstar] = 1.0
    return xq.to(dtype).contiguous(), xkv.to(dtype).contiguous(), w, S


def planted_gain(D):
    """The gain of planted(): with unit-scale K, a query gain k[l*] has logit gain |k|^2 / sqrt(D) ~ gain sqrt(D) at l* and
    ~ gain N(0, 1) elsewhere; 12 / sqrt(D) + 2 puts the planted key >= 12 natural units above the typical other key at every D
    of the cases: T[n][l*] near 1 on S and near 0 off it."""
    return 12.0 / math.sqrt(D) + 2.0


class WordTokenizer:
    """A whitespace tokenizer with CLIP's frame: BOS, one id per word (`snowboard` splits in two, as BPE would), EOS, then padding
    with the EOS id, as the SD1.5 tokenizer pads.  tokenize(str) -> (1, length) ids."""
    BOS, EOS = 1000, 1001

    def __init__(self, length=12):
        self.length, self.vocab = length, {}

    def __call__(self, prompt):
        ids = [self.BOS]
        for wd in prompt.lower().split():
            for piece in (("snow", "board") if wd == "snowboard" else (wd,)):
                ids.append(self.vocab.setdefault(piece, len(self.vocab) + 1))
        ids = ids[:self.length - 1] + [self.EOS]
        return torch.tensor([ids + [self.EOS] * (self.length - len(ids))])


def oracle_text_operands(unet, forward, target_block, target_layer):
    """The oracle's restatement of UNetEngine.qkv_text's xq / xkv for ONE image: (xq [2][N][C], xkv [2][L][2C]) f32.  unet: the
    oracle U-Net (oracle/cpu_ref.py, unchanged); forward(): runs its full forward on the image (cpu_ref.features(..., full=True) or
    features_xl).  The tapped block is the one whose attn1 is tap_module's; a forward pre-hook on its attn2 sees norm2's output and
    the context, and attn2.qkv projects them."""
    attn1 = unet.tap_module(target_block, target_layer)
    block = next(m for m in unet.modules() if getattr(m, "attn1", None) is attn1)
    store = {}

    def pre_hook(mod, args, kwargs):
        q, k, v = mod.qkv(args[0], kwargs["encoder_hidden_states"])
        flat = lambda t: t.transpose(1, 2).reshape(t.shape[0], t.shape[2], -1)            # noqa: E731  (B,H,N,D) -> [B][N][H*D]
        store["xq"], store["xkv"] = flat(q), torch.cat([flat(k), flat(v)], -1)

    hd = block.attn2.register_forward_pre_hook(pre_hook, with_kwargs=True)
    try:
        forward()
    finally:
        hd.remove()
    return store["xq"], store["xkv"]
