"""Region transfer (csrc/transfer.hip: transfer_part_kernel + transfer_fold_kernel behind dsim_pair_region_transfer) restated in
float64, with a per-entry bound on the kernels' f32 arithmetic, shared by tests/test_transfer_host.py and tests/test_gpu_transfer.py.
Not a conftest: import it like tests/_align64.py.

THE DEFINITION.  With Pm exactly as tests/_align64.py defines it (the softmax over ALL keys, the mean over the B CFG halves and the H
heads) and w_x[j] = byte / 255 of feature image x's token j,
    mass[p][0][i] = sum_j Pm_ab[i][j] w_b[j]      mass[p][1][u] = sum_t Pm_ba[u][t] w_a[t]
for pair p = (a, b).  mass64() is _align64.direction64's Pm contracted with w in float64.

THE BOUND, term by term from the kernels' rounding points (u32 = 2^-24, first order; p = P_bh, r_bh[i] = sum_j p_ij w_j).  The
arithmetic per query row and (b, h): e_ij = exp2(fma(s_ij, c, -m c)) from the alignments' logits; per 64-key tile and lane half the
sums psum = sum e and nsum = fmaf(e, w, nsum) from 0, joined to the running sums as l = fmaf(l, alpha, psum), num = fmaf(num, alpha,
nsum); the halves added; r_bh = num / l; mass = (sum_bh r_bh, ascending) * (1 / (B H)).
  * e_ij has _align64's relative error rho_ij = a_ij + 2 u32 gap_ij + 2^-23 (the f32 accumulation of the products, the f32 scale,
    v_exp_f32); the running maximum is a reference point that cancels between num and l.
  * the denominator l = sum_j e_ij carries sum_j p_ij rho_ij and its own summation: 31 adds per lane and tile, one fused
    rescale-and-add per tile (4 u32 for the factor alpha, 1 for the fma) and the add of the two halves:
        den_i = sum_j p_ij rho_ij + (33 + 5 ntiles) u32                   (_align64's den without its reciprocal: there is none here)
  * the numerator num = sum_j e_ij w_j carries sum_j p_ij w_j rho_ij relative to l, and of its own: the weight's rounding
    (float)byte / 255.0f, 1 u32; 32 fmas per lane and tile (the first one rounds the product: one more than l's 31 adds), the same
    rescale and half add as l: (34 + 5 ntiles) u32; the division num / l, correctly rounded, counted as 2 u32 as _align64 counts its
    reciprocal.  Together (37 + 5 ntiles) u32 r_bh.  [Taking _align64's den_i as it stands, (35 + 5 ntiles), and (35 + 5 ntiles + 4)
    here would count a reciprocal in den_i that this arithmetic does not make, and two roundings for the weight and the product where
    the fma makes one: the counts above are those of the arithmetic as written, and the tighter ones.]
        |dr_bh[i]| <= sum_j p_ij w_j (rho_ij + den_i) + (37 + 5 ntiles) u32 r_bh[i]
  * the head sum: B H f32 adds of partial sums that never exceed B H mass, the factor 1 / (B H) rounded once and multiplied once:
    (B H + 2) u32 mass.
  * arguments below -126 flush to zero in exp2, and so may the products behind them: 2^-124 per key, N keys.
        bound_i = mean_bh [sum_j p_ij w_j (rho_ij + den_i)] + (37 + 5 ntiles) u32 mean_bh r_bh[i] + (B H + 2) u32 mass_i + N 2^-124
No constant is fitted to what the kernels return."""
import math

import torch

from tests import _align64 as A

U32, LAM, EXP2_REL, FLOOR, KT = A.U32, A.LAM, A.EXP2_REL, A.FLOOR, A.KT


def direction_mass64(qa, kb, w_bytes, H, with_bound=True):
    """(mass, bound) [N] float64 of one direction: qa, kb [B][N][H*D] in the compute dtype, w_bytes [N] uint8 (the key image's); or
    [S][N] each for S weight sets [S][N] at once (the probabilities and their error terms are computed once)"""
    w = (w_bytes.double() / 255.0).t() if w_bytes.ndim == 2 else w_bytes.double() / 255.0       # [N] or [N][S]
    Pm, _ = A.direction64(qa, kb, H, with_bound=False)
    mass = Pm @ w
    if not with_bound:
        return (mass.t() if w.ndim == 2 else mass), None
    Q, K = A._heads(qa, H), A._heads(kb, H)
    BH, N, D = Q.shape
    t = Q @ K.transpose(1, 2) / math.sqrt(D)
    P = torch.softmax(t, -1)
    a = (Q.abs() @ K.abs().transpose(1, 2)) * (LAM * U32)          # (_align64's a: sqrt(D) of the sum over 1 / sqrt(D) of the scale)
    gap = t.max(-1, keepdim=True).values - t
    rho = a + 2 * U32 * gap + EXP2_REL
    ntiles = -(-N // KT)
    den = (P * rho).sum(-1, keepdim=True) + (33 + 5 * ntiles) * U32
    r = P @ w                                                       # [BH][N]
    first = ((P * (rho + den)) @ w).mean(0)
    bound = first + (37 + 5 * ntiles) * U32 * r.mean(0) + (BH + 2) * U32 * mass + N * FLOOR
    return (mass.t(), bound.t()) if w.ndim == 2 else (mass, bound)


def mass64(q, k, weights, pairs, H, with_bound=True):
    """(mass, bound): float64 [n_pairs][2][N] each (bound None without with_bound).  q, k: CPU [n][B][N][H*D]; weights: uint8 [n][N],
    or S weight sets [S][n][N] at once: [S][n_pairs][2][N] each"""
    out, bnd = [], []
    for ia, ib in pairs:
        rows = [direction_mass64(q[ia], k[ib], weights[..., ib, :], H, with_bound),
                direction_mass64(q[ib], k[ia], weights[..., ia, :], H, with_bound)]
        out.append(torch.stack([r[0] for r in rows], -2))
        if with_bound:
            bnd.append(torch.stack([r[1] for r in rows], -2))
    return torch.stack(out, -3), (torch.stack(bnd, -3) if with_bound else None)


def _fma32(a, b, c):
    """fma of f32 tensors: the product of two f32 values is exact in float64, the sum rounds once more at 2^-53"""
    return (a.double() * b.double() + c.double()).float()


def direction_mass32(qa, kb, w_bytes, H):
    """The kernels' arithmetic in plain float32 torch, [N] f32: the logits of an f32 matmul, the f32 scale as an fma, the online
    maximum over 64-key tiles, the two running sums with their fused rescale, the division and the ascending head sum.  (The order
    inside a tile's sums is torch's, and the product e w rounds on its own: both inside the bound's counts.)"""
    Q, K = A._heads(qa, H).float(), A._heads(kb, H).float()
    BH, N, D = Q.shape
    c = torch.tensor((1.0 / math.sqrt(D)), dtype=torch.float32) * torch.tensor(1.4426950408889634, dtype=torch.float32)
    w = w_bytes.float() / torch.tensor(255.0, dtype=torch.float32)
    total = torch.zeros(N, dtype=torch.float32)
    for bh in range(BH):
        s = Q[bh] @ K[bh].t()                                        # [N][N] f32
        mc = torch.full((N,), float("inf"), dtype=torch.float32)
        l = torch.zeros(N, dtype=torch.float32)
        num = torch.zeros(N, dtype=torch.float32)
        for j0 in range(0, N, KT):
            st = s[:, j0:j0 + KT]
            mc_new = torch.minimum(mc, -st.max(-1).values * c)
            alpha = torch.exp2(mc_new - mc)
            mc = mc_new
            e = torch.exp2(_fma32(st, c.expand_as(st), mc[:, None].expand_as(st)))
            l = _fma32(l, alpha, e.sum(-1))
            num = _fma32(num, alpha, (e * w[j0:j0 + KT]).sum(-1))
        total = total + num / l
    return total * (torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(BH), dtype=torch.float32))


def random_bytes(n, N, seed):
    """uint8 [n][N] uniform in 0 .. 255, zeros and 255s included"""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, N), generator=g, dtype=torch.uint8)


def binary_bytes(n, N, seed):
    """uint8 [n][N] of 0 / 255, each half the time"""
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(0, 2, (n, N), generator=g, dtype=torch.uint8) * 255)
