"""A float64 restatement of the region maps and the region alignments (include/diffsim_amd.h, dsim_pair_score_maps_regions and
dsim_pair_align_regions), shared by the region map tests.  Not a conftest: import it like tests/_region64.py.

Every image i has a token region R_i (a mask row); its rows are taken in ascending token order.

REGION MAPS.  Per pair and direction the two SDPAs of tests/_region64.Region64 (float64 on the gathered rows, outputs rounded to the
pipeline dtype) and tests/_tail64.products64 on them give the per-token local and contrib of the |R_query| region tokens; they are
scattered to the full grid of N tokens, zeros elsewhere.  score = 0.5 * contrib.sum().  A pair with an empty region: score NaN, maps
zero.

REGION ALIGNMENTS.  Per pair and direction tests/_align64.direction64 on the gathered rows gives Pm (|R_q|, |R_k|) and its bound;
both are scattered to the full (N, N) grid, zeros outside R_q x R_k.  direction64 counts the key tiles of its bound from the QUERY
count (it was written for Nq = Nk); its den term is (35 + 5 ntiles) u32 per probability, so the key count's tiles are put in their
place: bound += 5 (ntiles(|R_k|) - ntiles(|R_q|)) u32 Pm, which is that term's difference summed through mean_bh p (rho + den)."""
import torch

from tests import _align64 as A
from tests._region64 import Region64
from tests._tail64 import products64


def rows_of(mask):
    """[ascending on-token indices (int64, CPU)] per mask row"""
    return [torch.nonzero(m.detach().cpu() != 0).flatten() for m in mask]


def region_maps64(q, k, v, mask, idx_a, idx_b, H, sim, out_dtype):
    """[(score, local (2, N), contrib (2, N))] float64 on the full grid for the pairs (idx_a[p], idx_b[p])"""
    t = Region64(q, k, v, mask, H, out_dtype)
    N = q.shape[2]
    out = []
    for a, b in zip(torch.as_tensor(idx_a).tolist(), torch.as_tensor(idx_b).tolist()):
        local = torch.zeros(2, N, dtype=torch.float64)
        contrib = torch.zeros(2, N, dtype=torch.float64)
        if len(t.rows[a]) == 0 or len(t.rows[b]) == 0:
            out.append((float("nan"), local, contrib))
            continue
        for d, (x, y) in enumerate(((a, b), (b, a))):
            lo, co = products64(t.attn(x, y), t.attn(x, x), sim)
            local[d, t.rows[x]] = lo
            contrib[d, t.rows[x]] = co
        out.append((0.5 * float(contrib.sum()), local, contrib))
    return out


def region_direction64(qa, kb, ra, rb, H, with_bound=True):
    """(Pm, bound) float64 (N, N) of one direction on the full grid: qa, kb [B][N][H*D] in the compute dtype, ra / rb the query /
    key image's ascending region rows.  Zero outside ra x rb (the bound too: those entries are written as zeros, exactly)."""
    N = qa.shape[1]
    Pm = torch.zeros(N, N, dtype=torch.float64)
    bound = torch.zeros(N, N, dtype=torch.float64) if with_bound else None
    if len(ra) and len(rb):
        pm, bd = A.direction64(qa.cpu().index_select(1, ra), kb.cpu().index_select(1, rb), H, with_bound)
        Pm[ra[:, None], rb[None, :]] = pm
        if with_bound:
            tiles = lambda n: -(-n // A.KT)          # noqa: E731
            bd = bd + 5 * (tiles(len(rb)) - tiles(len(ra))) * A.U32 * pm
            bound[ra[:, None], rb[None, :]] = bd
    return Pm, bound


def region_align64(q, k, mask, pairs, H, with_bound=True):
    """(Pm, bound): float64 [n_pairs][2][N][N] each on the full grid (bound None without with_bound)"""
    rows = rows_of(mask)
    out, bnd = [], []
    for ia, ib in pairs:
        ds = [region_direction64(q[ia], k[ib], rows[ia], rows[ib], H, with_bound),
              region_direction64(q[ib], k[ia], rows[ib], rows[ia], H, with_bound)]
        out.append(torch.stack([d[0] for d in ds]))
        if with_bound:
            bnd.append(torch.stack([d[1] for d in ds]))
    return torch.stack(out), (torch.stack(bnd) if with_bound else None)


def region_outputs64(Pm, rows_q, rows_k, grid_w):
    """(match int64 (N,), weight (N,), expect (N, 2)) of one direction's full-grid Pm (N, N): the argmax over the key region (the
    lowest token on a tie), its probability, the soft-argmax in full-grid coordinates; the off values at the off query tokens (all
    tokens when a region is empty)"""
    N = Pm.shape[-1]
    match = torch.full((N,), -1, dtype=torch.int64)
    weight = torch.zeros(N, dtype=torch.float64)
    expect = torch.full((N, 2), -1.0, dtype=torch.float64)
    if len(rows_q) and len(rows_k):
        sub = Pm[rows_q][:, rows_k]
        m, w, _ = A.outputs64(sub, grid_w)
        match[rows_q] = rows_k[m]
        weight[rows_q] = w
        j = rows_k.double()
        coords = torch.stack([torch.div(j, grid_w, rounding_mode="floor"), j % grid_w], -1)
        expect[rows_q] = sub @ coords
    return match, weight, expect
