"""A float64 restatement of the soft region maps and the soft region alignments (include/diffsim_amd.h,
dsim_pair_score_maps_weights and dsim_pair_align_weights), shared by their tests.  Not a conftest: import it like
tests/_regionmap64.py, which it equals exactly where every weight byte is 0 or 255.

Every image i has a byte m_i[t] per token, w = m / 255; its rows of non-zero weight are taken in ascending token order.

SOFT MAPS.  Per pair and direction the two biased SDPAs of tests/_soft64.Soft64 (float64 on the gathered rows with ln w of the key
image's rows added to the logits, outputs rounded to the pipeline dtype).  local is tests/_tail64.products64's local on them: the
token's own value, its own weight not applied.  contrib is Soft64.direction's per-row term: the weighted one, whose sum is the
direction's soft value.  Both are scattered to the full grid of N tokens, zeros elsewhere; score = 0.5 * contrib.sum().  A pair with
an image of byte sum 0: score NaN, maps zero.

SOFT ALIGNMENTS.  tests/_align64.direction64's definition on the gathered rows with ln w_b[j] added to the logit of key j:
    P_bh[i][j] = softmax over the listed j of ( Q_a[i] . K_b[j] / sqrt(D) + ln w_b[j] ),     Pm = mean over (b, h).
THE BOUND is tests/_align64.py's, term by term, with what the bias adds.  The kernels keep the RAW running maximum m and compute
exp2(fma(s, c, -m c) + lb[j]), lb = log2(w) from a table rounded once to f32, |lb| <= 7.995:
  * gap_ij is the raw gap, max_j t_ij - t_ij over the listed keys (the reference point the kernels use; any reference point cancels);
  * the table entry: one rounding of |lb| <= 8 in log2 units, u32 8 ln 2 in natural units;
  * the added f32 addition: one more rounding of an exponent argument that is at most 8 larger in magnitude (log2 units) than the
    unbiased one: u32 (gap_ij + 8 ln 2) in natural units.
So rho_ij = a_ij + 3 u32 gap_ij + 16 ln 2 u32 + 2^-23 where _align64 has a_ij + 2 u32 gap_ij + 2^-23.  The numerators are at most 1
(a bias is <= 0) and the maximal raw key's is at least 2^-8, so the denominator and the flush floor are _align64's; its tile count is
the key count's.  With every byte 255 the three additions vanish only in the kernel, not in this bound: it is a bound, not a fit."""
import math

import torch

from tests import _align64 as A
from tests._soft64 import Soft64
from tests._tail64 import products64


def rows_of(weights):
    """[ascending indices of the tokens of non-zero weight (int64, CPU)] per weight row"""
    return [torch.nonzero(m.detach().cpu() != 0).flatten() for m in weights]


def soft_maps64(q, k, v, weights, idx_a, idx_b, H, sim, out_dtype):
    """[(score, local (2, N), contrib (2, N))] float64 on the full grid for the pairs (idx_a[p], idx_b[p])"""
    t = Soft64(q, k, v, weights, H, out_dtype)
    N = q.shape[2]
    out = []
    for a, b in zip(torch.as_tensor(idx_a).tolist(), torch.as_tensor(idx_b).tolist()):
        local = torch.zeros(2, N, dtype=torch.float64)
        contrib = torch.zeros(2, N, dtype=torch.float64)
        if len(t.rows[a]) == 0 or len(t.rows[b]) == 0:
            out.append((float("nan"), local, contrib))
            continue
        for d, (x, y) in enumerate(((a, b), (b, a))):
            local[d, t.rows[x]] = products64(t.attn(x, y), t.attn(x, x), sim)[0]
            contrib[d, t.rows[x]] = t.direction(x, y, sim)
        out.append((0.5 * float(contrib.sum()), local, contrib))
    return out


def soft_direction64(qa, kb, ra, rb, wb, H, with_bound=True):
    """(Pm, bound) float64 (N, N) of one direction on the full grid: qa, kb [B][N][H*D] in the compute dtype, ra / rb the query / key
    image's ascending rows of non-zero weight, wb the key image's weight bytes (N,).  Zero outside ra x rb (the bound too)."""
    N = qa.shape[1]
    Pm = torch.zeros(N, N, dtype=torch.float64)
    bound = torch.zeros(N, N, dtype=torch.float64) if with_bound else None
    if len(ra) == 0 or len(rb) == 0:
        return Pm, bound
    Q, K = A._heads(qa.cpu().index_select(1, ra), H), A._heads(kb.cpu().index_select(1, rb), H)
    BH, _, D = Q.shape
    t = Q @ K.transpose(1, 2) / math.sqrt(D)
    lnw = torch.log(wb.detach().cpu()[rb].double() / 255.0)
    P = torch.softmax(t + lnw, -1)
    pm = P.mean(0)
    Pm[ra[:, None], rb[None, :]] = pm
    if with_bound:
        a = (Q.abs() @ K.abs().transpose(1, 2)) * (A.LAM * A.U32)
        gap = t.max(-1, keepdim=True).values - t
        rho = a + 3 * A.U32 * gap + 16 * math.log(2.0) * A.U32 + A.EXP2_REL
        ntiles = -(-len(rb) // A.KT)
        den = (P * rho).sum(-1, keepdim=True) + (35 + 5 * ntiles) * A.U32
        bound[ra[:, None], rb[None, :]] = (P * (rho + den)).mean(0) + (BH + 2) * A.U32 * pm + A.FLOOR
    return Pm, bound


def soft_align64(q, k, weights, pairs, H, with_bound=True):
    """(Pm, bound): float64 [n_pairs][2][N][N] each on the full grid (bound None without with_bound)"""
    rows = rows_of(weights)
    out, bnd = [], []
    for ia, ib in pairs:
        ds = [soft_direction64(q[ia], k[ib], rows[ia], rows[ib], weights[ib], H, with_bound),
              soft_direction64(q[ib], k[ia], rows[ib], rows[ia], weights[ia], H, with_bound)]
        out.append(torch.stack([d[0] for d in ds]))
        if with_bound:
            bnd.append(torch.stack([d[1] for d in ds]))
    return torch.stack(out), (torch.stack(bnd) if with_bound else None)
